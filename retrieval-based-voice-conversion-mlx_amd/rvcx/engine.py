"""Device engine: one rvcx context (weights + workspace in HBM) driven through the C-ABI.

torch is used only for device memory and the current HIP stream; every computation runs in
librvcx.so (HIP kernels for gfx950).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Mapping, Optional

import numpy as np

from . import _lib
from .config import SYNTH_48K_V2, SynthConfig
from .engine_kernels import KernelTestMixin, _ptr
from .weights import normalize_state


def hubert_frames(n: int) -> int:
    """HuBERT feature rows for n samples at 16 kHz (the seven valid convs of its feature encoder); 0 when too short."""
    for k, s in ((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2)):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


class Engine(KernelTestMixin):
    """Owns an ``rvcx_ctx`` on one GPU. Not thread-safe (one host thread at a time). The product methods
    (include/rvcx.h) are here; the kernel-level test wrappers (include/rvcx_test.h) come from KernelTestMixin."""

    def __init__(self, device: int = 0):
        import torch

        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("rvcx needs a ROCm GPU: torch.cuda.is_available() is False")
        self.torch = torch
        self.device_index = int(device)
        self.device = torch.device(f"cuda:{self.device_index}")
        ctx = ctypes.c_void_p()
        rc = self.lib.rvcx_create(ctypes.byref(ctx), self.device_index)
        if rc != 0:
            raise _lib.RvcxError(rc, f"rvcx_create(device={device}) failed")
        self.ctx = ctx
        # the voice bank (rvcx_voice_*): per voice id its SynthConfig and whether its synthesizer is loaded; voice 0
        # exists from the start and is current. synth_cfg and loaded["synth"] follow the current voice.
        self._voices = {0: {"cfg": None, "loaded": False}}
        self._voice = 0
        self.loaded = {"synth": False, "hubert": False, "rmvpe": False, "crepe": None, "fcpe": None}
        self.fcpe_cfg = None

    @property
    def synth_cfg(self) -> Optional[SynthConfig]:
        return self._voices[self._voice]["cfg"]

    @synth_cfg.setter
    def synth_cfg(self, cfg):
        self._voices[self._voice]["cfg"] = cfg

    # ------------------------------------------------------------------ voice bank
    @property
    def voice(self) -> int:
        """The current voice: the one every synthesizer, pipeline and index method acts on."""
        return self._voice

    @property
    def voice_ids(self):
        return sorted(self._voices)

    def select_voice(self, voice: int):
        """rvcx_voice_select: host only (no device call, no copy). RvcxError(RVCX_E_INVALID) for an unknown or freed
        id."""
        self._check(self.lib.rvcx_voice_select(self.ctx, int(voice)), "voice_select")
        self._voice = int(voice)
        self.loaded["synth"] = self._voices[self._voice]["loaded"]

    def add_voice(self, state: Mapping[str, np.ndarray], cfg: SynthConfig = SYNTH_48K_V2, index=None) -> int:
        """A new resident voice: the synthesizer `state` under `cfg` and, optionally, its feature index (the bytes of
        a faiss IndexIVFFlat file). Returns its id; the current voice is the same before and after."""
        v = ctypes.c_int(0)
        self._check(self.lib.rvcx_voice_new(self.ctx, ctypes.byref(v)), "voice_new")
        vid, back = int(v.value), self._voice
        self._voices[vid] = {"cfg": None, "loaded": False}
        self.select_voice(vid)
        try:
            self.load_synth(state, cfg)
            if index is not None:
                self.index_load(index)
        except Exception:
            self.select_voice(back)
            self.free_voice(vid)
            raise
        self.select_voice(back)
        return vid

    def voice_info(self, voice: Optional[int] = None) -> dict:
        """rvcx_voice_info of any live voice (None: the current one): its SynthConfig as loaded here, ready, the index
        (dict(d, ntotal, nlist, nprobe) or None), weight_bytes (the packed tensors) and split_bytes (the pre-split
        weight images built from them so far)."""
        vid = self._voice if voice is None else int(voice)
        d = _lib.VoiceDesc()
        self._check(self.lib.rvcx_voice_info(self.ctx, vid, ctypes.byref(d)), "voice_info")
        index = None
        if d.index_ntotal or d.index_nlist:
            index = {"d": d.index_d, "ntotal": d.index_ntotal, "nlist": d.index_nlist, "nprobe": d.index_nprobe}
        return {"id": vid, "cfg": self._voices[vid]["cfg"], "ready": bool(d.ready), "sr": int(d.synth.sr),
                "upp": int(np.prod([d.synth.upsample_rates[i] for i in range(d.synth.n_upsample)], dtype=np.int64)),
                "index": index, "weight_bytes": int(d.weight_bytes), "split_bytes": int(d.split_bytes)}

    def free_voice(self, voice: int):
        """rvcx_voice_free: synchronises the device and releases the voice's tensors, split images and index.
        RvcxError(RVCX_E_STATE) for voice 0 and the current voice."""
        self._check(self.lib.rvcx_voice_free(self.ctx, int(voice)), "voice_free")
        self._voices.pop(int(voice), None)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rvcx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.rvcx_last_error(self.ctx)
            raise _lib.RvcxError(rc, f"{what}: {msg.decode() if msg else ''}")

    def check_device_status(self):
        """Synchronise the current stream and raise RvcxError(RVCX_E_HIP) if a kernel of an earlier call raised
        a device-side fault flag (e.g. the RMVPE BiGRU hand-off timed out: that call's outputs are invalid)."""
        self._check(self.lib.rvcx_device_status(self.ctx, self.stream()), "device status")

    def host(self, t):
        """Device tensor -> numpy at the API edge: synchronises, then raises RvcxError if a kernel of this (or an
        earlier) call raised a device-side fault flag, so a faulted result never leaves as data."""
        self.check_device_status()
        return t.cpu().numpy()

    def stream(self) -> int:
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _dev(self, x, dtype):
        t = self.torch
        if isinstance(x, t.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return t.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=self.device).contiguous()

    def _opt(self, x, dtype, *shape):
        """An optional argument on the device (reshaped when a shape is given); None stays None (a null pointer)."""
        if x is None:
            return None
        return self._dev(x, dtype).reshape(*shape) if shape else self._dev(x, dtype)

    @staticmethod
    def _seed(seed: int):
        return ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF)

    def _pad_rows(self, audios, dtype):
        """Rows of any lengths -> (a zero-padded [B, longest] device image, the rows' lengths); (None, []) for no rows."""
        t = self.torch
        rows = [self._dev(a, dtype).reshape(-1) for a in audios]
        ns = [int(r.numel()) for r in rows]
        if not rows:
            return None, ns
        a = t.zeros((len(rows), max(ns)), dtype=dtype, device=self.device)
        for b, r in enumerate(rows):
            a[b, : ns[b]] = r
        return a, ns

    def _need_fcpe(self):
        if self.fcpe_cfg is None:
            raise _lib.RvcxError(-5, "fcpe weights not loaded (Engine.load_fcpe)")

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _synth_desc(cfg: SynthConfig):
        d = _lib.SynthDesc()
        d.inter_channels, d.hidden_channels, d.filter_channels = cfg.inter_channels, cfg.hidden_channels, \
            cfg.filter_channels
        d.n_heads, d.n_layers, d.kernel_size = cfg.n_heads, cfg.n_layers, cfg.kernel_size
        d.n_resblocks = len(cfg.resblock_kernel_sizes)
        d.n_dilations = len(cfg.resblock_dilation_sizes[0])
        for j, k in enumerate(cfg.resblock_kernel_sizes):
            d.resblock_kernel_sizes[j] = k
            for m, dd in enumerate(cfg.resblock_dilation_sizes[j]):
                d.resblock_dilation_sizes[j][m] = dd
        d.n_upsample = len(cfg.upsample_rates)
        for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            d.upsample_rates[i] = u
            d.upsample_kernel_sizes[i] = k
        d.upsample_initial_channel = cfg.upsample_initial_channel
        d.spk_embed_dim, d.gin_channels, d.sr = cfg.spk_embed_dim, cfg.gin_channels, cfg.sr
        d.text_enc_hidden_dim = cfg.text_enc_hidden_dim
        d.no_f0 = 0 if cfg.use_f0 else 1
        if cfg.vocoder not in _lib.VOCODERS:
            raise ValueError(f"unknown vocoder {cfg.vocoder!r}; expected one of {sorted(_lib.VOCODERS)}")
        d.vocoder = _lib.VOCODERS[cfg.vocoder]
        return d

    def set_synth_config(self, cfg: SynthConfig = SYNTH_48K_V2):
        d = self._synth_desc(cfg)
        self._check(self.lib.rvcx_set_synth_config(self.ctx, ctypes.byref(d)), "set_synth_config")
        self.synth_cfg = cfg

    def upload_state(self, model: int, state: Mapping[str, np.ndarray]):
        """Upload a fused fp32 state dict (reference names and layouts) and finalize it."""
        for name, arr in state.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (ctypes.c_int64 * max(1, a.ndim))(*a.shape)
            self._check(self.lib.rvcx_upload(self.ctx, model, name.encode(), a.ctypes.data, shape, a.ndim),
                        f"upload {name}")
        self._check(self.lib.rvcx_finalize(self.ctx, model), "finalize")

    def load_synth(self, state: Mapping[str, np.ndarray], cfg: SynthConfig = SYNTH_48K_V2):
        self.set_synth_config(cfg)
        st = {k: v for k, v in normalize_state(state).items() if not k.startswith("enc_q.")}
        self.upload_state(_lib.RVCX_MODEL_SYNTH, st)
        self.loaded["synth"] = self._voices[self._voice]["loaded"] = True

    def load_hubert(self, state: Mapping[str, np.ndarray]):
        st = {k: v for k, v in normalize_state(state).items() if k != "masked_spec_embed"}
        self.upload_state(_lib.RVCX_MODEL_HUBERT, st)
        self.loaded["hubert"] = True

    def load_rmvpe(self, state: Mapping[str, np.ndarray]):
        self.upload_state(_lib.RVCX_MODEL_RMVPE, normalize_state(state))
        self.loaded["rmvpe"] = True

    def load_crepe(self, state: Mapping[str, np.ndarray], key=None):
        """CREPE weights under torchcrepe's names (rvcx.weights.load_crepe_weights); the context holds one CREPE
        model at a time (full or tiny, told apart by conv1's filter count). `key` names what was loaded so callers
        can skip a reload."""
        self.upload_state(_lib.RVCX_MODEL_CREPE, {k: v for k, v in state.items() if not k.endswith("num_batches_tracked")})
        self.loaded["crepe"] = key if key is not None else ("full" if np.shape(state["conv1.weight"])[0] == 1024
                                                           else "tiny")

    def crepe(self, audio, f0_min: float = 50.0, f0_max: float = 1100.0, threshold: float = 0.1,
              want_periodicity: bool = False, want_probs: bool = False, semantics: str = "mlx", dither=None):
        """CREPE.get_f0 (rvc_mlx/lib/mlx/crepe.py:282-325): audio [N] (16 kHz) -> f0 fp32 [1 + N//160] on device
        (and the filtered periodicity [F], the probabilities [F, 360]). semantics="rvc": rvc/'s CREPE.get_f0
        (torchcrepe.predict + viterbi, rvc/lib/predictors/f0.py:31-55; rvcx_crepe_ex); dither: its [F] cents noise
        (torchcrepe draws scipy.stats.triang(c=0.5, loc=-20, scale=40)), None = none."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        n = a.numel()
        F = 1 + n // 160
        f0 = t.empty((F,), dtype=t.float32, device=self.device)
        per = t.empty((F,), dtype=t.float32, device=self.device) if want_periodicity else None
        probs = t.empty((F, 360), dtype=t.float32, device=self.device) if want_probs else None
        fo = ctypes.c_int64(0)
        sem = {"mlx": 0, "rvc": 1}[semantics]
        d = self._opt(dither, t.float32, -1)
        if d is not None and d.numel() != F:
            raise ValueError(f"dither needs {F} values")
        self._check(self.lib.rvcx_crepe_ex(self.ctx, a.data_ptr(), n, float(f0_min), float(f0_max), float(threshold),
                                           sem, _ptr(d), f0.data_ptr(), _ptr(per), _ptr(probs), F, ctypes.byref(fo),
                                           self.stream()), "crepe")
        out = [f0]
        if want_periodicity:
            out.append(per)
        if want_probs:
            out.append(probs)
        return out[0] if len(out) == 1 else tuple(out)

    def crepe_decode(self, probs, f0_min: float = 50.0, f0_max: float = 1100.0, threshold: float = 0.1,
                     semantics: str = "rvc", dither=None):
        """rvcx_crepe_decode: the decode + filters alone on probabilities [F][360] -> (f0 [F], periodicity [F])."""
        t = self.torch
        p = self._dev(probs, t.float32).contiguous()
        F = int(p.shape[0])
        f0 = t.empty((F,), dtype=t.float32, device=self.device)
        per = t.empty((F,), dtype=t.float32, device=self.device)
        d = self._opt(dither, t.float32, -1)
        self._check(self.lib.rvcx_crepe_decode(self.ctx, p.data_ptr(), F, float(f0_min), float(f0_max),
                                               float(threshold), {"mlx": 0, "rvc": 1}[semantics], _ptr(d),
                                               f0.data_ptr(), per.data_ptr(), self.stream()), "crepe_decode")
        return f0, per

    def load_fcpe(self, state: Mapping[str, np.ndarray], config: Mapping, key=None):
        """An FCPE checkpoint's ``model`` state dict and ``config`` (rvc/lib/predictors/FCPE.py:731-756;
        rvcx.weights.load_fcpe_weights): the sizes go to rvcx_set_fcpe_config, the weights (dense_out's weight-norm
        fused) to RVCX_MODEL_FCPE. `key` names what was loaded so callers can skip a reload."""
        from .weights import check_fcpe_state, fcpe_sizes

        st = check_fcpe_state(state, config)
        z = fcpe_sizes(config)
        d = _lib.FcpeDesc()
        d.sampling_rate, d.n_fft, d.win_size, d.hop_size, d.num_mels = z["sampling_rate"], z["n_fft"], z["win_size"], \
            z["hop_size"], z["num_mels"]
        d.fmin, d.fmax = float(z["fmin"]), float(z["fmax"])
        d.n_layers, d.n_chans, d.out_dims = z["n_layers"], z["n_chans"], z["out_dims"]
        self._check(self.lib.rvcx_set_fcpe_config(self.ctx, ctypes.byref(d)), "set_fcpe_config")
        self.upload_state(_lib.RVCX_MODEL_FCPE, st)
        self.fcpe_cfg = z
        self.loaded["fcpe"] = key if key is not None else True

    _FCPE_DECODERS = {"local_argmax": 0, "argmax": 1}

    def _fcpe_frames(self, n: int) -> int:
        """Frames FCPEInfer gives for n samples (Wav2Mel.extract_mel, FCPE.py:805-813)."""
        z = self.fcpe_cfg
        win, hop = z["win_size"], z["hop_size"]
        pl = (win - hop) // 2
        pr = max((win - hop + 1) // 2, win - n - pl)
        fs = (n + pl + pr - win) // hop + 1
        nf = n // hop + 1
        return fs + 1 if nf > fs else nf

    def fcpe(self, audio, threshold: float = 0.006, decoder: str = "local_argmax", interp_uv: bool = False,
             pad_to=None, want_salience: bool = False, sample_rate=None):
        """FCPEInfer.__call__ (rvc/lib/predictors/FCPE.py:758-764) on device: audio [N] at the model's sampling rate
        -> f0 fp64 [N // hop + 1], zeros where the frame maximum <= threshold (and the salience [F, out_dims]).
        interp_uv: FCPEF0Predictor.post_process follows (:877-902; nearest expansion to pad_to frames, linear
        interpolation through the unvoiced ones) -> fp64 [pad_to or F]. sample_rate, when given, must be the
        model's: Wav2Mel's resampling branch (:795-803) is not built."""
        self._need_fcpe()
        if sample_rate is not None and int(sample_rate) != self.fcpe_cfg["sampling_rate"]:
            raise ValueError(f"fcpe: audio at {sample_rate} Hz, the model's mel runs at "
                             f"{self.fcpe_cfg['sampling_rate']} Hz (resampling is not supported)")
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        n = a.numel()
        F = self._fcpe_frames(n)
        n_out = int(pad_to) if (interp_uv and pad_to) else F
        f0 = t.empty((n_out,), dtype=t.float64, device=self.device)
        sal = t.empty((F, self.fcpe_cfg["out_dims"]), dtype=t.float32, device=self.device) if want_salience else None
        fo = ctypes.c_int64(0)
        self._check(self.lib.rvcx_fcpe(self.ctx, a.data_ptr(), n, float(threshold), self._FCPE_DECODERS[decoder],
                                       1 if interp_uv else 0, int(pad_to or 0), f0.data_ptr(), _ptr(sal), n_out,
                                       ctypes.byref(fo), self.stream()), "fcpe")
        assert fo.value == n_out, (fo.value, n_out)
        return (f0, sal) if want_salience else f0

    def fcpe_batch(self, audio, threshold: float = 0.006, decoder: str = "local_argmax", want_salience: bool = False):
        """rvcx_fcpe_b: FCPEInfer.__call__ for B streams in one batched forward. audio [B, n] at the model's sampling
        rate -> the raw track f0 fp64 [B, n // hop + 1], zeros where a frame's maximum <= threshold (and the salience
        [B, F, out_dims]). Each row is computed as rvcx_fcpe computes it alone: padding, statistics and the attention's
        sums are per stream."""
        self._need_fcpe()
        t = self.torch
        a = self._dev(audio, t.float32)
        if a.dim() != 2:
            raise ValueError("fcpe_batch: audio [B, n]")
        a = a.contiguous()
        B, n = int(a.shape[0]), int(a.shape[1])
        F = self._fcpe_frames(n)
        f0 = t.empty((B, F), dtype=t.float64, device=self.device)
        sal = t.empty((B, F, self.fcpe_cfg["out_dims"]), dtype=t.float32, device=self.device) if want_salience else None
        self._check(self.lib.rvcx_fcpe_b(self.ctx, a.data_ptr(), n, n, B, float(threshold), self._FCPE_DECODERS[decoder],
                                         f0.data_ptr(), _ptr(sal), self.stream()), "fcpe_b")
        return (f0, sal) if want_salience else f0

    def fcpe_batch_v(self, audios, threshold: float = 0.006, decoder: str = "local_argmax",
                     want_salience: bool = False):
        """audios: a list of [N_b] arrays (at the model's sampling rate) of any lengths -> a list of the raw tracks f0
        fp64 [N_b // hop + 1] on device (and the list of saliences [F_b, out_dims]), from one ragged pass over all rows
        (rvcx_fcpe_batch_v: each row is `fcpe`'s on that row alone, up to summation order; equal lengths are
        `fcpe_batch`'s bits, one row `fcpe`'s)."""
        self._need_fcpe()
        t = self.torch
        a, ns = self._pad_rows(audios, t.float32)
        if a is None:
            return ([], []) if want_salience else []
        B, lda = a.shape
        F, nb = self._fcpe_frames(lda), self.fcpe_cfg["out_dims"]
        f0 = t.empty((B, F), dtype=t.float64, device=self.device)
        sal = t.empty((B, F, nb), dtype=t.float32, device=self.device) if want_salience else None
        F_arr = (ctypes.c_int64 * B)()
        self._check(self.lib.rvcx_fcpe_batch_v(self.ctx, a.data_ptr(), (ctypes.c_int64 * B)(*ns), lda, B,
                                               float(threshold), self._FCPE_DECODERS[decoder], f0.data_ptr(), F, F_arr,
                                               _ptr(sal), F, self.stream()), "fcpe_batch_v")
        f0s = [f0[b, : int(F_arr[b])] for b in range(B)]
        if not want_salience:
            return f0s
        return f0s, [sal[b, : int(F_arr[b])] for b in range(B)]

    def fcpe_decode(self, salience, threshold: float = 0.006, decoder: str = "local_argmax", interp_uv: bool = False,
                    pad_to=None):
        """rvcx_fcpe_decode: the cents decoder (+ post_process) alone on salience [F][out_dims] -> f0 fp64."""
        self._need_fcpe()
        t = self.torch
        p = self._dev(salience, t.float32).reshape(-1, self.fcpe_cfg["out_dims"]).contiguous()
        F = int(p.shape[0])
        n_out = int(pad_to) if (interp_uv and pad_to) else F
        f0 = t.empty((n_out,), dtype=t.float64, device=self.device)
        self._check(self.lib.rvcx_fcpe_decode(self.ctx, p.data_ptr(), F, float(threshold),
                                              self._FCPE_DECODERS[decoder], 1 if interp_uv else 0, int(pad_to or 0),
                                              f0.data_ptr(), self.stream()), "fcpe_decode")
        return f0

    @property
    def upp(self) -> int:
        return int(self.lib.rvcx_synth_upp(self.ctx))

    # ------------------------------------------------------------------ compute
    def hubert(self, audio, version: str = "v2"):
        """audio [N] (16 kHz) -> feats [L, 768] (v2) / [L, 256] (v1), fp32 on device."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        n = a.numel()
        cap = n // 320 + 8
        D = 256 if version == "v1" else 768
        out = t.empty((cap, D), dtype=t.float32, device=self.device)
        rows = ctypes.c_int64(0)
        self._check(self.lib.rvcx_hubert(self.ctx, a.data_ptr(), n, 1 if version == "v1" else 2, out.data_ptr(), cap,
                                         ctypes.byref(rows), self.stream()), "hubert")
        return out[: rows.value]

    def rmvpe(self, audio, thred: float = 0.03, want_hidden: bool = False):
        """audio [N] (16 kHz) -> f0 fp64 [1 + N//160] on device (and salience [F, 360])."""
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        n = a.numel()
        F = 1 + n // 160
        f0 = t.empty((F,), dtype=t.float64, device=self.device)
        hid = t.empty((F, 360), dtype=t.float32, device=self.device) if want_hidden else None
        fo = ctypes.c_int64(0)
        self._check(self.lib.rvcx_rmvpe(self.ctx, a.data_ptr(), n, float(thred), f0.data_ptr(), F, ctypes.byref(fo),
                                        _ptr(hid), self.stream()), "rmvpe")
        return (f0, hid) if want_hidden else f0

    def hubert_batch(self, audio, version: str = "v2"):
        """audio [B, N] (16 kHz, equal lengths) -> feats [B, L, D] on device in one batched pass."""
        t = self.torch
        a = self._dev(audio, t.float32)
        B, n = int(a.shape[0]), int(a.shape[1])
        D = 256 if version == "v1" else 768
        cap = n // 320 + 8
        out = t.empty((B, cap, D), dtype=t.float32, device=self.device)
        rows = ctypes.c_int64(0)
        self._check(self.lib.rvcx_hubert_batch(self.ctx, a.data_ptr(), n, n, B, 1 if version == "v1" else 2,
                                               out.data_ptr(), cap, ctypes.byref(rows), self.stream()), "hubert_batch")
        L = rows.value
        return out.reshape(-1)[: B * L * D].reshape(B, L, D)

    def hubert_batch_v(self, audios, version: str = "v2", ld_rows: Optional[int] = None):
        """audios: a list of [N_b] arrays (16 kHz) of any lengths -> a list of feats [L_b, D] on device, from one
        batched pass over all rows (each row's frames are `hubert`'s on that row alone, up to summation order).
        ld_rows: frames between two rows' blocks in the output buffer (default: the longest row's frame count)."""
        t = self.torch
        a, ns = self._pad_rows(audios, t.float32)
        if a is None:
            return []
        B, lda = a.shape
        D = 256 if version == "v1" else 768
        cap = max(1, hubert_frames(lda)) if ld_rows is None else int(ld_rows)
        out = t.empty((B, cap, D), dtype=t.float32, device=self.device)
        n_arr = (ctypes.c_int64 * B)(*ns)
        L_arr = (ctypes.c_int64 * B)()
        self._check(self.lib.rvcx_hubert_batch_v(self.ctx, a.data_ptr(), n_arr, lda, B, 1 if version == "v1" else 2,
                                                 out.data_ptr(), cap, L_arr, self.stream()), "hubert_batch_v")
        return [out[b, : int(L_arr[b])] for b in range(B)]

    def rmvpe_batch(self, audio, thred: float = 0.03, want_hidden: bool = False):
        """audio [B, N] (16 kHz, equal lengths) -> f0 fp64 [B, 1 + N//160] (and salience [B, F, 360])."""
        t = self.torch
        a = self._dev(audio, t.float32)
        B, n = int(a.shape[0]), int(a.shape[1])
        F = 1 + n // 160
        f0 = t.empty((B, F), dtype=t.float64, device=self.device)
        hid = t.empty((B, F, 360), dtype=t.float32, device=self.device) if want_hidden else None
        fo = ctypes.c_int64(0)
        self._check(self.lib.rvcx_rmvpe_batch(self.ctx, a.data_ptr(), n, n, B, float(thred), f0.data_ptr(), F,
                                              ctypes.byref(fo), _ptr(hid), self.stream()), "rmvpe_batch")
        return (f0, hid) if want_hidden else f0

    def rmvpe_batch_v(self, audios, thred: float = 0.03, want_hidden: bool = False):
        """audios: a list of [N_b] arrays (16 kHz) of any lengths -> a list of f0 fp64 [1 + N_b//160] on device (and
        the list of saliences [F_b, 360]), from one ragged pass over all rows (rvcx_rmvpe_batch_v: each row is `rmvpe`'s
        on that row alone, up to summation order)."""
        t = self.torch
        a, ns = self._pad_rows(audios, t.float32)
        if a is None:
            return ([], []) if want_hidden else []
        B, lda = a.shape
        F = 1 + lda // 160
        f0 = t.empty((B, F), dtype=t.float64, device=self.device)
        hid = t.empty((B, F, 360), dtype=t.float32, device=self.device) if want_hidden else None
        F_arr = (ctypes.c_int64 * B)()
        self._check(self.lib.rvcx_rmvpe_batch_v(self.ctx, a.data_ptr(), (ctypes.c_int64 * B)(*ns), lda, B, float(thred),
                                                f0.data_ptr(), F, F_arr, _ptr(hid), F, self.stream()), "rmvpe_batch_v")
        f0s = [f0[b, : int(F_arr[b])] for b in range(B)]
        if not want_hidden:
            return f0s
        return f0s, [hid[b, : int(F_arr[b])] for b in range(B)]

    def rmvpe_decode(self, hidden, thred: float = 0.03):
        """RMVPE0Predictor.decode on device: salience [F, 360] -> f0 fp64 [F]."""
        t = self.torch
        h = self._dev(hidden, t.float32).reshape(-1, 360)
        f0 = t.empty((h.shape[0],), dtype=t.float64, device=self.device)
        self._check(self.lib.rvcx_rmvpe_decode(self.ctx, h.data_ptr(), h.shape[0], float(thred), f0.data_ptr(),
                                               self.stream()), "rmvpe_decode")
        return f0

    def f0_post(self, f0, semitones: float):
        """Pitch shift + coarse quantisation on device: (coarse int32, pitchf fp32, f0 fp64)."""
        t = self.torch
        f = self._dev(f0, t.float64).reshape(-1)
        F = f.numel()
        coarse = t.empty((F,), dtype=t.int32, device=self.device)
        pitchf = t.empty((F,), dtype=t.float32, device=self.device)
        fs = t.empty((F,), dtype=t.float64, device=self.device)
        self._check(self.lib.rvcx_f0_post(self.ctx, f.data_ptr(), F, float(semitones), coarse.data_ptr(),
                                          pitchf.data_ptr(), fs.data_ptr(), self.stream()), "f0_post")
        return coarse, pitchf, fs

    def _synth_args(self, phone, lengths, pitch, pitchf, sid, eps_z, eps_src):
        """What the two Synthesizer.infer entries share: B, T, the pointers (None: null) of the device arguments before
        the noise (phone, lengths, pitch, pitchf, sid) and of the noise (eps_z, eps_src), the tensors themselves (to be
        kept alive over the call), out [B, T upp] and a maker of [B, T, I] outputs."""
        t = self.torch
        ph = self._dev(phone, t.float32)
        B, T = int(ph.shape[0]), int(ph.shape[1])
        args = (ph, self._dev(lengths, t.int32).reshape(B), self._opt(pitch, t.int32, B, T),
                self._opt(pitchf, t.float32, B, T), self._dev(sid, t.int32).reshape(B))
        noise = (self._opt(eps_z, t.float32), self._opt(eps_src, t.float32))
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        I = self.synth_cfg.inter_channels
        return (B, T, [_ptr(x) for x in args], [_ptr(x) for x in noise], args + noise, out,
                lambda: t.empty((B, T, I), dtype=t.float32, device=self.device))

    def synth_infer(self, phone, lengths, pitch, pitchf, sid, eps_z=None, eps_src=None, seed: int = 0,
                    want_latents: bool = False):
        B, T, args, noise, _keep, out, latent = self._synth_args(phone, lengths, pitch, pitchf, sid, eps_z, eps_src)
        zp, z = (latent(), latent()) if want_latents else (None, None)
        self._check(self.lib.rvcx_synth_infer(self.ctx, B, T, *args, *noise, self._seed(seed), out.data_ptr(), _ptr(zp),
                                              _ptr(z), self.stream()), "synth_infer")
        return (out, zp, z) if want_latents else out

    def synth_infer_ex(self, phone, lengths, pitch, pitchf, sid, rate=None, eps_z=None, eps_src=None, seed: int = 0):
        """Synthesizer.infer with rate and the full return value (rvcx_synth_infer_ex): -> (out [B][T' upp],
        z_p [B][T'][I], z [B][T'][I], m_p [B][T][I], logs_p [B][T][I]) with T' = T - int(T (1 - rate))."""
        B, T, args, noise, _keep, out, latent = self._synth_args(phone, lengths, pitch, pitchf, sid, eps_z, eps_src)
        zp, z, mp, lp = latent(), latent(), latent(), latent()
        I = self.synth_cfg.inter_channels
        tn = ctypes.c_int(0)
        self._check(self.lib.rvcx_synth_infer_ex(self.ctx, B, T, *args, -1.0 if rate is None else float(rate), *noise,
                                                 self._seed(seed), out.data_ptr(), zp.data_ptr(), z.data_ptr(),
                                                 mp.data_ptr(), lp.data_ptr(), ctypes.byref(tn), self.stream()),
                    "synth_infer_ex")
        Tn = int(tn.value)
        return (out.reshape(-1)[: B * Tn * self.upp].reshape(B, Tn * self.upp), zp.reshape(-1)[: B * Tn * I].reshape(B, Tn, I),
                z.reshape(-1)[: B * Tn * I].reshape(B, Tn, I), mp, lp)

    def dec_only(self, z, f0, sid, eps_src=None, seed: int = 0):
        t = self.torch
        zz = self._dev(z, t.float32)
        B, I, T = zz.shape
        f = self._opt(f0, t.float32, B, T)
        sd = self._dev(sid, t.int32).reshape(B)
        es = self._opt(eps_src, t.float32)
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_dec_only(self.ctx, B, T, zz.data_ptr(), _ptr(f), sd.data_ptr(), _ptr(es),
                                           self._seed(seed), out.data_ptr(),
                                           self.stream()), "dec_only")
        return out

    def voice_conversion(self, audio_pad, pitch, pitchf, sid: int, protect: float, eps_z=None, eps_src=None,
                         seed: int = 0, index_rate: float = 0.0):
        """HuBERT -> x2 upsample -> protect -> Synthesizer.infer on one padded chunk (device in/out)."""
        t = self.torch
        a = self._dev(audio_pad, t.float32).reshape(-1)
        n = a.numel()
        pc = self._opt(pitch, t.int32, -1)
        pf = self._opt(pitchf, t.float32, -1)
        cap = (n // 160) * self.upp
        out = t.empty((cap,), dtype=t.float32, device=self.device)
        no = ctypes.c_int64(0)
        ez = self._opt(eps_z, t.float32)
        es = self._opt(eps_src, t.float32)
        self._check(self.lib.rvcx_voice_conversion(self.ctx, a.data_ptr(), n, _ptr(pc), _ptr(pf), int(sid),
                                                   float(protect), float(index_rate), _ptr(ez), _ptr(es),
                                                   self._seed(seed), out.data_ptr(), cap,
                                                   ctypes.byref(no), self.stream()), "voice_conversion")
        return out[: no.value]

    # ------------------------------------------------------------------ whole pipeline
    def set_highpass(self, b, a, zi, sos=None):
        """The pipeline's high-pass (pipeline.py:22-27) as transfer function (+ lfilter_zi) and, when given,
        as second-order sections (run as a chunk-parallel scan)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        a = np.ascontiguousarray(a, dtype=np.float64)
        zi = np.ascontiguousarray(zi, dtype=np.float64)
        self._check(self.lib.rvcx_set_highpass(self.ctx, b.ctypes.data, a.ctypes.data, zi.ctypes.data, len(a) - 1),
                    "set_highpass")
        if sos is not None:
            q = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 6)
            self._check(self.lib.rvcx_set_highpass_sos(self.ctx, q.ctypes.data, q.shape[0]), "set_highpass_sos")
        self._hp = (b, a, zi)

    def set_pipeline_highpass(self, sr: int = 16000):
        """signal.butter(N=5, Wn=48, btype='high', fs=16000) as rvc/infer/pipeline.py:22-27 designs it."""
        from scipy import signal

        b, a = signal.butter(N=5, Wn=48, btype="high", fs=sr)
        sos = signal.butter(N=5, Wn=48, btype="high", fs=sr, output="sos")
        self.set_highpass(b, a, signal.lfilter_zi(b, a), sos)

    def highpass_pad(self, audio, t_pad: int):
        """filtfilt + reflect pad on device: fp64 [n] -> (fp64, fp32) [n + 2 t_pad]."""
        t = self.torch
        a = self._dev(audio, t.float64).reshape(-1)
        n = a.numel()
        p64 = t.empty((n + 2 * t_pad,), dtype=t.float64, device=self.device)
        p32 = t.empty((n + 2 * t_pad,), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_highpass_pad(self.ctx, a.data_ptr(), n, int(t_pad), p64.data_ptr(), p32.data_ptr(),
                                               self.stream()), "highpass_pad")
        return p64, p32

    _RESAMPLE_DTYPES = {"float64": 0, "float32": 1, "int16": 2, "int32": 3}

    def resample_poly(self, rows, up: int, down: int, dtype=None, channels: int = 1):
        """scipy.signal.resample_poly(x, up, down) of every row in one launch (rvcx_resample_poly_v), decode and channel
        downmix included. rows: a list of arrays / tensors (or one) of float64, float32, int16 (scaled by 2^-15) or
        int32 (2^-31) samples, [n] mono or [n, channels] interleaved frames, all of one dtype (`dtype`, a numpy dtype
        or name; None: the first row's). Returns a list of fp64 device tensors [ceil(n up / down)] (one tensor for one
        row); they are views of one zero-padded [B, ld] buffer, so they can go on into a batched pass as they are.
        The filter is rvcx.resample.taps(up, down), kept on the device per (up, down)."""
        from . import resample as rs

        t = self.torch
        single = not isinstance(rows, (list, tuple))
        rows = [rows] if single else list(rows)
        if not rows:
            return []
        ch = int(channels)
        name = str(np.dtype(dtype)) if dtype is not None else \
            str(rows[0].dtype).replace("torch.", "")
        if name not in self._RESAMPLE_DTYPES:
            raise TypeError(f"resample_poly takes float64, float32, int16 or int32 samples, not {name}")
        tdt = getattr(t, name)
        up, down = rs.reduce(up, down)
        B = len(rows)
        ns = []
        for r in rows:
            if r.ndim > 2 or (r.ndim == 2 and int(r.shape[1]) != ch) or (r.ndim == 1 and int(r.shape[0]) % ch):
                raise ValueError(f"resample_poly: a row of shape {tuple(r.shape)} does not hold frames of {ch} channels")
            ns.append(int(r.shape[0]) if r.ndim == 2 else int(r.shape[0]) // ch)
        ldx = max(ns)
        if B == 1:
            x = self._dev(rows[0], tdt).reshape(-1)
        elif not any(isinstance(r, t.Tensor) for r in rows):  # host rows: one padded image, one copy
            hx = np.zeros((B, ldx * ch), dtype=name)
            for b, r in enumerate(rows):
                hx[b, : ns[b] * ch] = np.asarray(r, dtype=name).reshape(-1)
            x = t.as_tensor(hx, device=self.device)
        else:
            x = t.zeros((B, ldx * ch), dtype=tdt, device=self.device)
            for b, r in enumerate(rows):
                x[b, : ns[b] * ch] = self._dev(r, tdt).reshape(-1)
        cache = self.__dict__.setdefault("_resample_taps", {})
        h = cache.get((up, down))
        if h is None:
            h = cache[(up, down)] = t.as_tensor(np.array(rs.taps(up, down)), device=self.device)
        ldy = max(rs.plan(n, up, down)[2] for n in ns)
        y = t.empty((B, ldy), dtype=t.float64, device=self.device)
        no = (ctypes.c_int64 * B)()
        self._check(self.lib.rvcx_resample_poly_v(self.ctx, x.data_ptr(), self._RESAMPLE_DTYPES[name], ch,
                                                  (ctypes.c_int64 * B)(*ns), ldx, B, up, down, h.data_ptr(),
                                                  h.numel(), y.data_ptr(), ldy, no, self.stream()), "resample_poly")
        out = [y[b, : int(no[b])] for b in range(B)]
        return out[0] if single else out

    def pipeline(self, audio, sid: int = 0, semitones: float = 0.0, protect: float = 0.33, t_pad: int = 16000,
                 t_pad_tgt: int = 48000, eps_z=None, eps_src=None, seed: int = 0, out=None, want_f0: bool = False):
        """One utterance (padded length <= t_max) through the whole device pipeline.
        audio: fp64 [n] @16 kHz (device tensor or numpy). Returns fp32 [n_out] on device."""
        t = self.torch
        a = self._dev(audio, t.float64).reshape(-1)
        n = a.numel()
        m = n + 2 * t_pad
        cap = (m // 160) * self.upp
        if out is None:
            out = t.empty((cap,), dtype=t.float32, device=self.device)
        f0 = t.empty((1 + m // 160,), dtype=t.float64, device=self.device) if want_f0 else None
        no = ctypes.c_int64(0)
        ez = self._opt(eps_z, t.float32)
        es = self._opt(eps_src, t.float32)
        self._check(self.lib.rvcx_pipeline(self.ctx, a.data_ptr(), n, int(sid), float(semitones), float(protect),
                                           int(t_pad), int(t_pad_tgt), _ptr(ez), _ptr(es),
                                           self._seed(seed), out.data_ptr(), out.numel(),
                                           ctypes.byref(no), _ptr(f0), self.stream()), "pipeline")
        res = out[: no.value]
        return (res, f0) if want_f0 else res

    def config_info(self) -> dict:
        """The effective configuration (rvcx_config_info): contraction arithmetic, whether RVCX_* developer knobs are
        honoured (RVCX_EXPERIMENTAL=1), and each RVCX_* variable of the environment."""
        import json

        n = ctypes.c_int64(0)
        self.lib.rvcx_config_info(self.ctx, None, 0, ctypes.byref(n))
        buf = ctypes.create_string_buffer(int(n.value) + 1)
        self._check(self.lib.rvcx_config_info(self.ctx, ctypes.cast(buf, ctypes.c_void_p), len(buf), ctypes.byref(n)),
                    "config_info")
        return json.loads(buf.value.decode())

    def workspace_bytes(self, n: int, B: int = 1, opts=None) -> int:
        """Device scratch a pipeline call of B utterances of n samples takes (rvcx_workspace_bytes: one call on zero
        audio from an empty pool; the pool is released after)."""
        o = opts if opts is not None else self.pipeline_opts()
        v = ctypes.c_int64(0)
        self._check(self.lib.rvcx_workspace_bytes(self.ctx, int(B), int(n), ctypes.byref(o), ctypes.byref(v),
                                                  self.stream()), "workspace_bytes")
        return int(v.value)

    def set_workspace(self, arena=None):
        """Carve the context's scratch from a caller-owned device tensor (rvcx_set_workspace; None: back to internal
        allocation). The tensor is kept referenced here for as long as it is attached."""
        base = 0 if arena is None else arena.data_ptr()
        nbytes = 0 if arena is None else arena.numel() * arena.element_size()
        self._check(self.lib.rvcx_set_workspace(self.ctx, ctypes.c_void_p(base or None), int(nbytes)),
                    "set_workspace")
        self._arena = arena

    def workspace_info(self):
        """(bytes the pool holds, arena bytes, arena bytes carved)."""
        v = [ctypes.c_int64(0) for _ in range(3)]
        self._check(self.lib.rvcx_workspace_info(self.ctx, *(ctypes.byref(x) for x in v)), "workspace_info")
        return tuple(int(x.value) for x in v)

    def pipeline_opts(self, **kw) -> "_lib.PipelineOpts":
        """rvcx_pipeline_opts with the C defaults, overridden by keyword (field names of the struct)."""
        o = _lib.PipelineOpts()
        self.lib.rvcx_pipeline_default_opts(ctypes.byref(o))
        names = {f[0] for f in _lib.PipelineOpts._fields_}
        for k, v in kw.items():
            if k not in names:
                raise TypeError(f"unknown pipeline option {k!r}")
            setattr(o, k, v)
        return o

    def pipeline_ex(self, audio, opts: "_lib.PipelineOpts", eps_z=None, eps_src=None, seed: int = 0, out=None,
                    want_f0: bool = False):
        """Pipeline.pipeline on device with long-input splitting, f0 adjustments and volume envelope.
        audio: fp64 [n] @16 kHz. Returns fp32 [n_out] on device (and the adjusted f0 when want_f0)."""
        t = self.torch
        a = self._dev(audio, t.float64).reshape(-1)
        n = a.numel()
        m = n + 2 * int(opts.t_pad)
        n_split = n // int(opts.t_center) if opts.t_max > 0 and opts.t_center > 0 else 0
        cap = (m // 160 + n_split + 2) * self.upp
        if out is None or out.numel() < cap:
            out = t.empty((cap,), dtype=t.float32, device=self.device)
        f0 = t.empty((1 + m // 160,), dtype=t.float64, device=self.device) if want_f0 else None
        no = ctypes.c_int64(0)
        ez = self._opt(eps_z, t.float32)
        es = self._opt(eps_src, t.float32)
        self._check(self.lib.rvcx_pipeline_ex(self.ctx, a.data_ptr(), n, ctypes.byref(opts), _ptr(ez), _ptr(es),
                                              self._seed(seed), out.data_ptr(), out.numel(),
                                              ctypes.byref(no), _ptr(f0), self.stream()), "pipeline_ex")
        res = out[: no.value]
        return (res, f0) if want_f0 else res

    def _pipeline_rows(self, a, ns, opts, sids, eps_z, eps_src, seed, out, want_f0, want_hidden, voices=None):
        """What rvcx_pipeline_batch and rvcx_pipeline_batch_v share: a [B, lda] fp64 on device, rows of ns samples
        (an int: the equal-length entry). voices: None, or a voice id per row, rows of one voice contiguous
        (rvcx_pipeline_batch_voices). Returns (out [B, ldo], n_out per row, f0 [B, F] or None, salience or None)."""
        t = self.torch
        B, lda = int(a.shape[0]), int(a.shape[1])
        m = lda + 2 * int(opts.t_pad)
        # the voices of one batch share the upsample product; the current voice need not be one of them
        ldo = (m // 160) * (self.upp if voices is None else self.voice_info(voices[0])["upp"])
        if out is None or out.numel() < B * ldo:
            out = t.empty((B, ldo), dtype=t.float32, device=self.device)
        out = out.reshape(-1)[: B * ldo].reshape(B, ldo)
        sid = np.broadcast_to(np.asarray(sids, dtype=np.int32), (B,))
        sarr = (ctypes.c_int32 * B)(*[int(v) for v in sid])
        ez = self._opt(eps_z, t.float32)
        es = self._opt(eps_src, t.float32)
        F = 1 + m // 160
        f0 = t.empty((B, F), dtype=t.float64, device=self.device) if want_f0 else None
        hid = t.empty((B, F, 360), dtype=t.float32, device=self.device) if want_hidden else None
        head = (self.ctx, a.data_ptr())
        mid = (lda, B, ctypes.byref(opts), sarr, _ptr(ez), _ptr(es), self._seed(seed),
               out.data_ptr(), ldo)
        if isinstance(ns, int):
            no = ctypes.c_int64(0)
            self._check(self.lib.rvcx_pipeline_batch(*head, ns, *mid, ctypes.byref(no), _ptr(f0), _ptr(hid),
                                                     self.stream()), "pipeline_batch")
            return out, [int(no.value)] * B, f0, hid
        no = (ctypes.c_int64 * B)()
        if voices is None:
            self._check(self.lib.rvcx_pipeline_batch_v(*head, (ctypes.c_int64 * B)(*ns), *mid, no, _ptr(f0), F,
                                                       self.stream()), "pipeline_batch_v")
        else:
            varr = (ctypes.c_int32 * B)(*[int(v) for v in voices])
            self._check(self.lib.rvcx_pipeline_batch_voices(*head, (ctypes.c_int64 * B)(*ns), *mid[:4], varr, *mid[4:],
                                                            no, _ptr(f0), F, self.stream()), "pipeline_batch_voices")
        return out, [int(v) for v in no], f0, hid

    def pipeline_batch(self, audio, opts: "_lib.PipelineOpts", sids=0, eps_z=None, eps_src=None, seed: int = 0,
                       out=None, want_f0: bool = False, want_hidden: bool = False):
        """B equal-length utterances (fp64 [B, n] @16 kHz, each within t_max) through one batched pass.
        Returns fp32 [B, n_out] on device (row b = Pipeline.pipeline of utterance b); with want_f0 / want_hidden
        also the rows' adjusted f0 fp64 [B, F] / RMVPE salience fp32 [B, F, 360]."""
        a = self._dev(audio, self.torch.float64)
        out, no, f0, hid = self._pipeline_rows(a, int(a.shape[1]), opts, sids, eps_z, eps_src, seed, out, want_f0,
                                               want_hidden)
        y = out[:, : no[0]]
        extra = [v for v, w in ((f0, want_f0), (hid, want_hidden)) if w]
        return (y, *extra) if extra else y

    def pipeline_frames(self, n: int, opts: "_lib.PipelineOpts") -> int:
        """Synthesizer frames of an utterance of n samples under opts: min((n + 2 t_pad) / 160, 2 L)."""
        m = int(n) + 2 * int(opts.t_pad)
        return min(m // 160, 2 * hubert_frames(m))

    def pipeline_batch_v(self, audios, opts: "_lib.PipelineOpts", sids=0, eps_z=None, eps_src=None, seed: int = 0,
                         want_f0: bool = False, voices=None):
        """Utterances of different lengths (a list of fp64 [n_b] arrays @16 kHz, each within t_max) through one
        batched pass (rvcx_pipeline_batch_v). Returns a list of fp32 [n_out_b] device tensors (row b =
        Pipeline.pipeline of utterance b); with want_f0 also the list of the rows' adjusted f0 (fp64 [F_b]).
        eps_z [B, inter, T_max] / eps_src [B, T_max * upp] with T_max = max pipeline_frames(n_b): row b consumes
        eps_z[b, :, :T_b] and eps_src[b, :T_b * upp].
        voices: None (every row on the current voice), one voice id, or one per row with the rows of one voice
        contiguous (rvcx_pipeline_batch_voices): HuBERT and the pitch network run once over all rows, retrieval and the
        synthesizer once per voice."""
        a, ns = self._pad_rows(audios, self.torch.float64)
        if a is None:
            return ([], []) if want_f0 else []
        B = len(ns)
        if voices is not None:
            voices = [int(v) for v in np.broadcast_to(np.asarray(voices, dtype=np.int64), (B,))]
        out, no, f0, _ = self._pipeline_rows(a, ns, opts, sids, eps_z, eps_src, seed, None, want_f0, False, voices)
        ys = [out[b, : no[b]] for b in range(B)]
        if not want_f0:
            return ys
        return ys, [f0[b, : 1 + (ns[b] + 2 * int(opts.t_pad)) // 160] for b in range(B)]

    def f0_autotune(self, f0, strength: float = 1.0, skip_unvoiced: bool = False):
        """Autotune.autotune_f0 on device; returns a new fp64 tensor."""
        t = self.torch
        f = self._dev(f0, t.float64).reshape(-1).clone()
        self._check(self.lib.rvcx_f0_autotune(self.ctx, f.data_ptr(), f.numel(), float(strength),
                                              1 if skip_unvoiced else 0, self.stream()), "f0_autotune")
        return f

    def spectral_gate(self, x, sr: int, prop_decrease, return_mask: bool = False):
        """The realtime path's noise gate (rvc/realtime/core.py:86-94: TorchGate(sr, prop_decrease=...), stationary,
        no noise clip) on device: x [B, n] or [n] fp32 -> [B, 256 * (n // 256)], the length torch.istft returns, as the
        reference's module does. prop_decrease: one strength in [0, 1] for every row, or one per row where a negative
        entry copies that row through (its first n_out samples are returned). return_mask: also the bins above their
        threshold, bool [B, 513, 1 + n // 256]. ValueError for a strength above 1."""
        t = self.torch
        xx = self._dev(x, t.float32)
        xx = xx.reshape(1, -1) if xx.dim() == 1 else xx.reshape(-1, xx.shape[-1])
        B, n = xx.shape
        p = np.broadcast_to(np.asarray(prop_decrease, dtype=np.float64), (B,))
        if not np.all(p <= 1.0):
            raise ValueError(f"prop_decrease must lie in [0, 1], got {prop_decrease!r}")
        strength = (ctypes.c_float * B)(*[float(v) for v in p])
        y = t.empty((B, n), dtype=t.float32, device=self.device)
        mask = t.zeros((B, 513, 1 + n // 256), dtype=t.uint8, device=self.device) if return_mask else None
        self._check(self.lib.rvcx_spectral_gate(self.ctx, xx.data_ptr(), B, n, xx.stride(0), int(sr), strength,
                                                y.data_ptr(), y.stride(0), _ptr(mask), self.stream()), "spectral_gate")
        y = y[:, : 256 * (n // 256)]
        return (y, mask.bool()) if return_mask else y

    # ------------------------------------------------------------------ feature index (FAISS IVFFlat)
    def index_load(self, data: bytes):
        """Parse a faiss IndexIVFFlat file image and keep it in HBM (faiss.read_index, pipeline.py:430-434)."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        self._check(self.lib.rvcx_index_load(self.ctx, buf, len(data)), "index_load")
        self.index_info()

    def index_unload(self):
        self._check(self.lib.rvcx_index_unload(self.ctx), "index_unload")

    def index_info(self):
        """-> dict(d, ntotal, nlist, nprobe), or None when no index is loaded."""
        v = [ctypes.c_int64(0) for _ in range(4)]
        rc = self.lib.rvcx_index_info(self.ctx, *[ctypes.byref(x) for x in v])
        if rc == -5:
            return None
        self._check(rc, "index_info")
        return dict(zip(("d", "ntotal", "nlist", "nprobe"), (x.value for x in v)))

    def index_set_nprobe(self, nprobe: int):
        self._check(self.lib.rvcx_index_set_nprobe(self.ctx, int(nprobe)), "index_set_nprobe")

    def index_search(self, x, k: int = 8):
        """index.search(x, k) on device -> (dist fp32 [n, k], ids int64 [n, k]) device tensors."""
        t = self.torch
        xx = self._dev(x, t.float32)
        xx = xx.reshape(-1, xx.shape[-1])
        n = xx.shape[0]
        dist = t.empty((n, k), dtype=t.float32, device=self.device)
        ids = t.empty((n, k), dtype=t.int64, device=self.device)
        self._check(self.lib.rvcx_index_search(self.ctx, xx.data_ptr(), n, int(k), dist.data_ptr(), ids.data_ptr(),
                                               self.stream()), "index_search")
        return dist, ids

    def index_reconstruct_n(self, i0: int, ni: int):
        info = self.index_info()
        if info is None:
            raise _lib.RvcxError(-5, "no feature index loaded")
        out = self.torch.empty((int(ni), info["d"]), dtype=self.torch.float32, device=self.device)
        self._check(self.lib.rvcx_index_reconstruct_n(self.ctx, int(i0), int(ni), out.data_ptr(), self.stream()),
                    "index_reconstruct_n")
        return out

    def index_retrieve(self, feats, index_rate: float):
        """Pipeline._retrieve_speaker_embeddings on device: feats [L, d] -> blended [L, d]."""
        t = self.torch
        f = self._dev(feats, t.float32)
        f = f.reshape(-1, f.shape[-1])
        out = t.empty_like(f)
        self._check(self.lib.rvcx_index_retrieve(self.ctx, f.data_ptr(), f.shape[0], f.shape[1], float(index_rate),
                                                 out.data_ptr(), self.stream()), "index_retrieve")
        return out

    # ------------------------------------------------------------------ feature index: build and write
    def index_build(self, x, nlist: int, niter: int = 10, nprobe: int = 1, seed: int = 0, init_rows=None):
        """index.train(x) + index.add(x) on device (extract_index.py:58-68): k-means over x [n, d] into nlist lists;
        the result becomes this engine's loaded index. init_rows: nlist distinct rows of x as the initial centroids
        (default: drawn from seed). -> index_info()."""
        t = self.torch
        xx = self._dev(x, t.float32)
        xx = xx.reshape(-1, xx.shape[-1])
        o = _lib.IndexBuildOpts()
        self._check(self.lib.rvcx_index_default_build_opts(ctypes.byref(o)), "index_default_build_opts")
        o.niter, o.nprobe, o.seed = int(niter), int(nprobe), int(seed)
        rows = None
        if init_rows is not None:
            rows = np.ascontiguousarray(init_rows, dtype=np.int64).reshape(-1)
            if rows.size != int(nlist):
                raise _lib.RvcxError(-1, f"index_build: init_rows holds {rows.size} rows, nlist is {nlist}")
            o.init_rows = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        self._check(self.lib.rvcx_index_build(self.ctx, xx.data_ptr(), xx.shape[0], xx.shape[1], int(nlist),
                                              ctypes.byref(o), self.stream()), "index_build")
        return self.index_info()

    def index_centroids(self):
        """The loaded index's coarse centroids -> fp32 [nlist, d] device tensor."""
        info = self.index_info()
        if info is None:
            raise _lib.RvcxError(-5, "no feature index loaded")
        out = self.torch.empty((info["nlist"], info["d"]), dtype=self.torch.float32, device=self.device)
        self._check(self.lib.rvcx_index_centroids(self.ctx, out.data_ptr(), self.stream()), "index_centroids")
        return out

    def index_save(self) -> bytes:
        """faiss.write_index of the loaded index (extract_index.py:70) -> the file's bytes."""
        nb = ctypes.c_int64(0)
        self._check(self.lib.rvcx_index_save(self.ctx, None, 0, ctypes.byref(nb)), "index_save")
        buf = ctypes.create_string_buffer(nb.value)
        self._check(self.lib.rvcx_index_save(self.ctx, buf, nb.value, ctypes.byref(nb)), "index_save")
        return buf.raw[:nb.value]

    # ------------------------------------------------------------------ kernel timing
    def profile(self, enable: bool):
        self._check(self.lib.rvcx_profile(self.ctx, 1 if enable else 0), "profile")

    def profile_read(self, with_ceiling: bool = False):
        """(summed conv-GEMM kernel ms, summed algorithmic FLOPs, launches) since the last read; with_ceiling adds
        the same launches' time at their arithmetic's MFMA ceiling (ms, rvcx_profile_read_ex)."""
        ms, fl, n, cm = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
        self._check(self.lib.rvcx_profile_read_ex(self.ctx, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n),
                                                  ctypes.byref(cm)), "profile_read")
        return (ms.value, fl.value, n.value, cm.value) if with_ceiling else (ms.value, fl.value, n.value)

    def profile_read_kinds(self):
        """((ms, flops, launches, ceiling_ms) totals, {kernel family: {ms, flops, ceiling_ms, bytes, launches}}) since
        the last read (rvcx_profile_read_kinds: grouped by the kernel each launch actually ran)."""
        K = 10  # RVCX_PROF_KINDS
        arr = lambda T: (T * K)()  # noqa: E731
        kms, kfl, kcm, kby, kn = arr(ctypes.c_double), arr(ctypes.c_double), arr(ctypes.c_double), \
            arr(ctypes.c_double), arr(ctypes.c_int64)
        ms, fl, n, cm = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
        self._check(self.lib.rvcx_profile_read_kinds(self.ctx, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n),
                                                     ctypes.byref(cm), K, kms, kfl, kcm, kby, kn), "profile_read_kinds")
        fam = {}
        for k in range(K):
            if kn[k]:
                fam[self.lib.rvcx_profile_kind_name(k).decode()] = {"ms": kms[k], "flops": kfl[k], "ceiling_ms": kcm[k],
                                                                    "bytes": kby[k], "launches": int(kn[k])}
        return (ms.value, fl.value, n.value, cm.value), fam
