"""RVC_MLX-compatible front end on MI355X (rvc_mlx/infer/infer_mlx.py:106-343).

``RVCX(model_path).infer(audio_input, audio_output, pitch, f0_method, index_path, index_rate,
volume_envelope, protect, f0_autotune, f0_autotune_strength)`` loads a voice model, converts a
WAV file and writes the result at the model's sample rate. Attributes kept from the reference:
``tgt_sr``, ``net_g``, ``hubert_model``, ``rmvpe_model``, ``pipeline``.

Model files (all loaded without executing anything from the file):
  * RVC ``.pth`` (``weight``/``config``/``version``; rvc/train/process/extract_model.py:57-109) via
    torch.load(weights_only=True), weight-norm pairs fused exactly like torch.
  * MLX ``.npz`` / ``.safetensors`` written by tools/convert_rvc_model.py (remapped names, MLX
    layouts, already fused) plus an optional sibling ``.json`` config list (infer_mlx.py:146-205).
HuBERT/ContentVec and RMVPE weights come from local files only (no download: the reference's
``load_embedding``/``from_pretrained`` fetch over the network, rvc/lib/utils.py:125-153): the MLX tree's
``hubert_mlx.npz`` / ``rmvpe_mlx.npz`` (tools/convert_hubert.py, tools/convert_rmvpe.py layouts) or the
torch ``pytorch_model.bin`` / ``model.safetensors`` / ``rmvpe.pt`` (``HUBERT_CANDIDATES``, ``RMVPE_CANDIDATES``).
"""
from __future__ import annotations

import contextlib
import json
import os
from typing import Dict, Mapping, Optional

import numpy as np

from ..config import SynthConfig
from ..engine import Engine
from ..weights import load_rvc_checkpoint, load_state_file, normalize_state, unmap_mlx_keys
from .models import HubertModel, RMVPE0Predictor, Synthesizer
from .pipeline import Config, PipelineRVCX, VoiceRef

# infer_mlx.py:130-176 defaults when an MLX file has no config (40 kHz v2)
_MLX_DEFAULT_40K = SynthConfig(upsample_rates=(10, 10, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), sr=40000)

# Searched relative to the working directory, the MLX tree's own files first, as RVC_MLX does
# (infer_mlx.py:258-264 for HuBERT; RMVPE0Predictor's default, rvc_mlx/lib/mlx/rmvpe.py:256-258), then the
# rvc/ torch files (rvc/lib/utils.py:125-153, RMVPE.py:429-434).
HUBERT_CANDIDATES = ("rvc_mlx/models/embedders/contentvec/hubert_mlx.npz",
                     "rvc/models/embedders/contentvec/hubert_mlx.npz",
                     "rvc/models/embedders/contentvec/pytorch_model.bin",
                     "rvc/models/embedders/contentvec/model.safetensors")
RMVPE_CANDIDATES = ("rvc_mlx/models/predictors/rmvpe_mlx.npz",
                    "rvc/models/predictors/rmvpe.pt")


def mlx_to_reference_state(weights: Mapping[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Undo tools/convert_rvc_model.py:340-392: names back to reference keys, MLX layouts back to torch
    (Conv1d (O,K,I) -> (O,I,K); ConvTranspose1d (O,K,I) -> (I,O,K); Conv2d (O,H,W,I) -> (O,I,H,W))."""
    names = unmap_mlx_keys(weights.keys())
    out = {}
    for k, v in weights.items():
        n = names[k]
        a = np.asarray(v, dtype=np.float32)
        if a.ndim == 4:
            a = a.transpose(0, 3, 1, 2)
        elif a.ndim == 3 and "emb_rel" not in n:
            a = a.transpose(2, 0, 1) if n.startswith("dec.ups.") else a.transpose(0, 2, 1)
        out[n] = np.ascontiguousarray(a)
    return out


def load_voice_model(path: str):
    """-> (fused reference-name state, SynthConfig, version)."""
    import dataclasses

    if path.endswith(".pth"):
        state, cfg_list, meta = load_rvc_checkpoint(path)
        version = meta.get("version") or "v1"
        cfg = SynthConfig.from_list(cfg_list)
        if version == "v1":
            cfg = dataclasses.replace(cfg, text_enc_hidden_dim=256)
        cfg = dataclasses.replace(cfg, use_f0=bool(meta.get("f0", 1)),
                                  vocoder=str(meta.get("vocoder") or "HiFi-GAN"))
        return state, cfg, version
    if path.endswith(".npz") or path.endswith(".safetensors"):
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                raw = {k: z[k] for k in z.files}
        else:
            from safetensors.numpy import load_file

            raw = load_file(path)
        state = normalize_state(mlx_to_reference_state(raw))
        cfg = _MLX_DEFAULT_40K
        cfg_path = os.path.splitext(path)[0] + ".json"
        if os.path.exists(cfg_path):
            cfg = SynthConfig.from_json(cfg_path)
        if "emb_g.weight" in state:
            import dataclasses

            cfg = dataclasses.replace(cfg, spk_embed_dim=int(state["emb_g.weight"].shape[0]))
        emb = state.get("enc_p.emb_phone.weight")
        version = "v1" if emb is not None and emb.shape[1] == 256 else "v2"
        if version == "v1":
            import dataclasses

            cfg = dataclasses.replace(cfg, text_enc_hidden_dim=256)
        return state, cfg, version
    raise ValueError(f"unsupported voice model format: {path}")


def _first_existing(cands):
    for c in cands:
        if os.path.exists(c):
            return c
    return None


def load_audio(file_path: str, sr: int = 16000, engine: Optional[Engine] = None):
    """WAV -> mono float64 @sr (infer_mlx.py:91-104; resampling by polyphase filtering). With an engine the samples
    go to the device as the file holds them and decode, downmix and resampling run there in one launch
    (load_audio_device): the result is an fp64 device tensor, equal to the host route's up to summation order."""
    if engine is not None:
        return load_audio_device([file_path], engine, sr)[0]
    from math import gcd

    from scipy import signal
    from scipy.io import wavfile

    rate, data = wavfile.read(file_path)
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
    data = np.asarray(data, dtype=np.float64)
    if data.ndim > 1:
        data = data.mean(axis=1)
    if rate != sr:
        g = gcd(int(rate), int(sr))
        data = signal.resample_poly(data, sr // g, int(rate) // g)
    return data


DEVICE_WAV_DTYPES = ("int16", "int32", "float32", "float64")  # what rvcx_resample_poly_v decodes


def load_audio_device(paths, engine: Engine, sr: int = 16000):
    """`load_audio` of every file on the device -> fp64 device tensors in input order. The files are grouped by
    (rate, channels, dtype) and each group is decoded, downmixed and resampled in one rvcx_resample_poly_v launch.
    A WAV of another sample type (uint8) goes through the host `load_audio` and is uploaded."""
    from scipy.io import wavfile

    out = [None] * len(paths)
    groups: Dict[tuple, list] = {}
    for i, p in enumerate(paths):
        rate, data = wavfile.read(p)
        if str(data.dtype) not in DEVICE_WAV_DTYPES:
            out[i] = engine._dev(load_audio(p, sr), engine.torch.float64)
            continue
        ch = 1 if data.ndim == 1 else int(data.shape[1])
        groups.setdefault((int(rate), ch, str(data.dtype)), []).append((i, data))
    for (rate, ch, dt), items in groups.items():
        ys = engine.resample_poly([d for _, d in items], sr, rate, dtype=dt, channels=ch)
        for (i, _), y in zip(items, ys):
            out[i] = y
    return out


class RVCX:
    def __init__(self, model_path: Optional[str] = None, config=None, hubert_path: Optional[str] = None,
                 rmvpe_path: Optional[str] = None, device: int = 0, semantics: str = "rvc", *,
                 synth_state: Optional[Mapping[str, np.ndarray]] = None, synth_cfg: Optional[SynthConfig] = None,
                 hubert_state: Optional[Mapping[str, np.ndarray]] = None,
                 rmvpe_state: Optional[Mapping[str, np.ndarray]] = None, version: str = "v2", fcpe_weights=None,
                 fcpe_threshold: float = 0.006):
        """fcpe_weights / fcpe_threshold: PipelineRVCX's (an FCPE checkpoint's path or its (state, config) pair, which
        f0_method "fcpe" runs under semantics "rvc"; without it that method raises)."""
        self.config = config
        self.model_path = model_path
        if synth_state is None:
            if model_path is None:
                raise ValueError("model_path or synth_state is required")
            synth_state, synth_cfg, version = load_voice_model(model_path)
        if hubert_state is None:
            hp = hubert_path or _first_existing(HUBERT_CANDIDATES)
            if hp is None:
                raise FileNotFoundError("HuBERT/ContentVec weights not found; pass hubert_path (no download)")
            hubert_state = load_state_file(hp)
        if rmvpe_state is None:
            rp = rmvpe_path or _first_existing(RMVPE_CANDIDATES)
            if rp is None:
                raise FileNotFoundError("RMVPE weights not found; pass rmvpe_path (no download)")
            rmvpe_state = load_state_file(rp)
        self.version = version
        self.engine = Engine(device)
        self.engine.load_synth(synth_state, synth_cfg or SynthConfig())
        self.engine.load_hubert(hubert_state)
        self.engine.load_rmvpe(rmvpe_state)
        self.tgt_sr = self.engine.synth_cfg.sr
        self.use_f0 = bool(self.engine.synth_cfg.use_f0)  # pitch_guidance of infer.py:300
        self.net_g = Synthesizer(self.engine)
        self.hubert_model = HubertModel(self.engine, version)
        self.rmvpe_model = RMVPE0Predictor(self.engine)
        self.pipeline_config = config or Config()
        self.pipeline = PipelineRVCX(self.tgt_sr, self.pipeline_config, self.hubert_model, self.rmvpe_model,
                                     semantics=semantics, fcpe_weights=fcpe_weights, fcpe_threshold=fcpe_threshold)
        # the resident voices by name: the constructor's model is the first and the default of every call
        self._voices: Dict[str, VoiceRef] = {}
        self.default_voice = self._register(self._voice_name(None, model_path, 0), 0, version, None)

    # ------------------------------------------------------------------ voices
    @staticmethod
    def _voice_name(name, model_path, vid) -> str:
        if name is not None:
            return str(name)
        return os.path.splitext(os.path.basename(model_path))[0] if model_path else f"voice{vid}"

    def _register(self, name, vid, version, index_path) -> str:
        if name in self._voices:
            raise ValueError(f"a voice named {name!r} is already resident")
        cfg = self.engine.voice_info(vid)["cfg"]
        self._voices[name] = VoiceRef(vid, cfg.sr, bool(cfg.use_f0), version, index_path)
        return name

    @property
    def voices(self):
        """The names of the resident voices, the constructor's first."""
        return list(self._voices)

    def add_voice(self, model_path: Optional[str] = None, *, synth_state=None, synth_cfg: Optional[SynthConfig] = None,
                  index_path: Optional[str] = None, name: Optional[str] = None, version: str = "v2") -> str:
        """Load another voice beside the ones resident: a checkpoint (model_path, as the constructor reads it) or a
        state dict with its SynthConfig, and optionally its .index file, used whenever a call on this voice gives no
        index_path of its own. HuBERT, the pitch networks and the workspace are shared. Returns the voice's name
        (`name`, else the model file's stem), which `voice=` / `voices=` of the conversion calls take."""
        if synth_state is None:
            if model_path is None:
                raise ValueError("model_path or synth_state is required")
            synth_state, synth_cfg, version = load_voice_model(model_path)
        if name is not None or model_path:  # refused before anything is loaded
            if self._voice_name(name, model_path, 0) in self._voices:
                raise ValueError(f"a voice named {self._voice_name(name, model_path, 0)!r} is already resident")
        vid = self.engine.add_voice(synth_state, synth_cfg or SynthConfig())
        return self._register(self._voice_name(name, model_path, vid), vid, version, index_path)

    def _ref(self, voice) -> VoiceRef:
        if voice is None:
            voice = self.default_voice
        if voice not in self._voices:
            raise KeyError(f"no resident voice named {voice!r} (have: {self.voices})")
        return self._voices[voice]

    @contextlib.contextmanager
    def _on(self, voice):
        """Run a call on a resident voice: the engine's current voice, tgt_sr, use_f0, version and the pipeline's
        output padding are that voice's inside, and what they were after."""
        v = self._ref(voice)
        back = (self.engine.voice, self.tgt_sr, self.use_f0, self.version, self.hubert_model.version,
                self.pipeline.tgt_sr)
        self.engine.select_voice(v.id)
        self.tgt_sr, self.use_f0, self.version = v.tgt_sr, v.pitch_guidance, v.version
        self.hubert_model.version = v.version
        self.pipeline.set_tgt_sr(v.tgt_sr)
        try:
            yield v
        finally:
            self.engine.select_voice(back[0])
            self.tgt_sr, self.use_f0, self.version, self.hubert_model.version = back[1:5]
            self.pipeline.set_tgt_sr(back[5])

    def convert(self, audio: np.ndarray, pitch=0, f0_method="rmvpe", index_path=None, index_rate=0.75,
                volume_envelope=1.0, protect=0.5, f0_autotune=False, f0_autotune_strength=1.0, sid=0,
                proposed_pitch=False, proposed_pitch_threshold=155.0, seed: int = 0,
                split_audio: bool = False, resample_sr: int = 0, voice=None) -> np.ndarray:
        """16 kHz mono audio (numpy, or a device tensor as load_audio(engine=) returns it) -> converted float32 audio
        @tgt_sr (the body of infer_mlx.py:287-336). split_audio converts the non-silent intervals one by one and
        merges them back with the gaps restored (rvc/infer/infer.py:282-316). resample_sr: the output's rate
        (`output_sr`); the output is resampled to it on the device when it is at least 16000 and not tgt_sr.
        voice: the resident voice to convert with (a name of `voices`; None: the constructor's). The output is at that
        voice's tgt_sr, and its own index_path (add_voice) is used when none is given here."""
        with self._on(voice) as v:
            return self._convert(audio, pitch, f0_method, index_path or v.file_index, index_rate, volume_envelope,
                                 protect, f0_autotune, f0_autotune_strength, sid, proposed_pitch,
                                 proposed_pitch_threshold, seed, split_audio, resample_sr)

    def _convert(self, audio, pitch, f0_method, index_path, index_rate, volume_envelope, protect, f0_autotune,
                 f0_autotune_strength, sid, proposed_pitch, proposed_pitch_threshold, seed, split_audio, resample_sr):
        from ..split import merge_audio, process_audio

        post = None if split_audio else self._resampler(resample_sr)
        chunks, intervals = process_audio(self.engine, audio, 16000) if split_audio else ([audio], None)
        outs = [self.pipeline.pipeline(self.hubert_model, self.net_g, sid, c, pitch, f0_method, index_path,
                                       index_rate, self.use_f0, volume_envelope, self.version, protect, f0_autotune,
                                       f0_autotune_strength, proposed_pitch, proposed_pitch_threshold, seed=seed,
                                       post=post)
                for c in chunks]
        if not split_audio:
            return outs[0]
        merged = merge_audio(chunks, outs, intervals, 16000, self.tgt_sr)
        post = self._resampler(resample_sr)  # the merged signal is resampled, not its pieces
        return merged if post is None else self.engine.host(post(merged))

    def output_sr(self, resample_sr: int = 0, voice=None) -> int:
        """The rate `convert(..., resample_sr=, voice=)` delivers: resample_sr when it is at least 16000 and differs
        from the voice's tgt_sr (the condition of rvc/infer/infer.py:279), else that tgt_sr. voice None: the voice of
        the call in progress, else the constructor's."""
        tgt = self.tgt_sr if voice is None else self._ref(voice).tgt_sr
        r = int(resample_sr or 0)
        return r if r >= 16000 and r != tgt else tgt

    def _resampler(self, resample_sr, tgt_sr=None):
        """The output stage of resample_sr: float32 @tgt_sr -> float32 @resample_sr on the device (fp64 arithmetic,
        rvcx_resample_poly_v), or None when the output stays at tgt_sr (None: the current voice's)."""
        tgt = self.tgt_sr if tgt_sr is None else int(tgt_sr)
        r = int(resample_sr or 0)
        sr = r if r >= 16000 and r != tgt else tgt
        if sr == tgt:
            return None
        eng = self.engine
        return lambda y: eng.resample_poly(eng._dev(y, eng.torch.float32).reshape(-1), sr, tgt).to(eng.torch.float32)

    def convert_many(self, audios, pitch=0, f0_method="rmvpe", index_path=None, index_rate=0.75, volume_envelope=1.0,
                     protect=0.5, f0_autotune=False, f0_autotune_strength=1.0, sid=0, proposed_pitch=False,
                     proposed_pitch_threshold=155.0, seed: int = 0, batch: Optional[int] = None,
                     max_pad: Optional[float] = None, noise_fn=None, ragged_f0: bool = False, resample_sr: int = 0,
                     voices=None):
        """`convert` over a list of 16 kHz utterances of any lengths -> the outputs in input order. Utterances of
        similar length share one batched pass (PipelineRVCX.pipeline_many: sorted by length, a batch filled while its
        shortest row is at least (1 - max_pad) of its longest, inputs above t_max converted alone). ragged_f0
        (f0_method "rmvpe" or "fcpe"): the rows of a batch also share one ragged pass of the pitch network. An
        utterance may be a device tensor; resample_sr as in `convert`.
        voices: one resident voice for every utterance, or one name per utterance in any order (None: the
        constructor's). Utterances of voices that can share a pass (same rate, upsampling, embedding width, pitch
        guidance and vocoder) are batched together: HuBERT and the pitch network run once over the batch, the
        synthesizer once per voice. Each output is at its voice's rate (`output_sr(resample_sr, voice)`)."""
        from .pipeline import DEFAULT_BATCH, DEFAULT_MAX_PAD

        audios = list(audios)
        kw = dict(seed=seed, batch=DEFAULT_BATCH if batch is None else batch,
                  max_pad=DEFAULT_MAX_PAD if max_pad is None else max_pad, noise_fn=noise_fn, ragged_f0=ragged_f0)
        if voices is None or isinstance(voices, str):
            with self._on(voices) as v:
                return self.pipeline.pipeline_many(
                    self.hubert_model, self.net_g, sid, audios, pitch, f0_method, index_path or v.file_index,
                    index_rate, self.use_f0, volume_envelope, self.version, protect, f0_autotune, f0_autotune_strength,
                    proposed_pitch, proposed_pitch_threshold, post=self._resampler(resample_sr), **kw)
        refs = [self._ref(n) for n in voices]
        if len(refs) != len(audios):
            raise ValueError(f"voices has {len(refs)} names for {len(audios)} utterances")
        post = {r.id: self._resampler(resample_sr, r.tgt_sr) for r in refs}
        return self.pipeline.pipeline_many(
            self.hubert_model, self.net_g, sid, audios, pitch, f0_method, index_path, index_rate, self.use_f0,
            volume_envelope, self.version, protect, f0_autotune, f0_autotune_strength, proposed_pitch,
            proposed_pitch_threshold, post=post, voices=refs, **kw)

    def infer_batch(self, input_dir, output_dir, device_load: bool = False, **kw):
        """convert_audio_batch (rvc/infer/infer.py:350-414) over the WAV files of input_dir: every file converted with
        the options of `convert_many` and written under the same name to output_dir (at resample_sr when that
        applies). Returns the output paths. device_load: the files are decoded and resampled on the device, each group
        of one (rate, channels, sample type) in one launch (load_audio_device), and stay there into the batched pass."""
        from scipy.io import wavfile

        names = sorted(f for f in os.listdir(input_dir) if f.lower().endswith(".wav"))
        files = [os.path.join(input_dir, f) for f in names]
        audios = load_audio_device(files, self.engine) if device_load else [load_audio(f) for f in files]
        voice = kw.pop("voice", None)  # one voice for the directory (convert_many's voices= with one name)
        outs = self.convert_many(audios, voices=voice, **kw)
        os.makedirs(output_dir, exist_ok=True)
        paths = []
        rate = self.output_sr(kw.get("resample_sr", 0), voice or self.default_voice)
        for f, y in zip(names, outs):
            paths.append(os.path.join(output_dir, f))
            wavfile.write(paths[-1], rate, np.asarray(y, dtype=np.float32))
        return paths

    def infer(self, audio_input, audio_output, pitch=0, f0_method="rmvpe", index_path=None, index_rate=0.75,
              volume_envelope=1.0, protect=0.5, f0_autotune=False, f0_autotune_strength=1.0, split_audio=False,
              device_load: bool = False, resample_sr: int = 0, voice=None):
        """device_load: the file is decoded and resampled to 16 kHz on the device (load_audio(engine=)).
        resample_sr: as in `convert`; the file is written at that rate. voice: as in `convert`."""
        from scipy.io import wavfile

        audio = load_audio(audio_input, engine=self.engine) if device_load else load_audio(audio_input)
        out = self.convert(audio, pitch, f0_method, index_path, index_rate, volume_envelope, protect, f0_autotune,
                           f0_autotune_strength, split_audio=split_audio, resample_sr=resample_sr, voice=voice)
        wavfile.write(audio_output, self.output_sr(resample_sr, voice or self.default_voice), out.astype(np.float32))
        return out

    def build_index(self, audio_paths_or_arrays, out_path: str, algorithm: str = "Auto", seed: int = 0,
                    device_load: bool = False, voice=None, **kw):
        """The .index file that index_rate > 0 needs, from the speaker's audio: the HuBERT features of every file or
        16 kHz array, as rvc/train/extract/extract.py:133-139 saves them (files whose features hold NaN are skipped),
        then rvc/train/process/extract_index.py:37-70 on device (rvcx.infer.index.build_index) and write. Returns
        the built IndexIVFFlat, which is the loaded index of `voice` (None: the constructor's voice). device_load: files
        are loaded on the device."""
        with self._on(voice):
            return self._build_index(audio_paths_or_arrays, out_path, algorithm, seed, device_load, **kw)

    def _build_index(self, audio_paths_or_arrays, out_path, algorithm, seed, device_load, **kw):
        from .index import build_index

        feats = []
        for a in audio_paths_or_arrays:
            if isinstance(a, (str, os.PathLike)):
                audio = load_audio(a, engine=self.engine) if device_load else load_audio(a)
            else:
                audio = np.asarray(a)
            f = self.engine.host(self.engine.hubert(audio, self.version))
            if np.isnan(f).any():
                continue
            feats.append(f)
        if not feats:
            raise ValueError("build_index: no usable audio (every file's features held NaN, or none was given)")
        index = build_index(self.engine, np.concatenate(feats, axis=0), algorithm=algorithm, seed=seed, **kw)
        index.write(out_path)
        return index

    def close(self):
        self.engine.close()


RVC_MLX = RVCX
