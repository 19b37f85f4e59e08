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
from .weights import normalize_state


def hubert_frames(n: int) -> int:
    """HuBERT feature rows for n samples at 16 kHz (the seven valid convs of its feature encoder); 0 when too short."""
    for k, s in ((10, 5), (3, 2), (3, 2), (3, 2), (3, 2), (2, 2), (2, 2)):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


class Engine:
    """Owns an ``rvcx_ctx`` on one GPU. Not thread-safe (one host thread at a time)."""

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
        self.synth_cfg: Optional[SynthConfig] = None
        self.loaded = {"synth": False, "hubert": False, "rmvpe": False, "crepe": None, "fcpe": None}
        self.fcpe_cfg = None

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

    def set_dec_window(self, on: bool):
        """The generator's output window on (the default) or off (rvcx_set_dec_window, include/rvcx_test.h): with it
        on, the pipelines and stream groups run the generator only over the frames their trim keeps. Outputs are
        bit-identical either way."""
        self._check(self.lib.rvcx_set_dec_window(self.ctx, 1 if on else 0), "set_dec_window")

    def dec_margin_frames(self, cfg: SynthConfig = None) -> int:
        """The generator's one-sided receptive field in frames for `cfg` (default: the loaded configuration): the
        margin the output window keeps per cut side (rvcx_dec_margin_frames). Host only."""
        d = self._synth_desc(cfg if cfg is not None else self.synth_cfg)
        m = ctypes.c_int32(0)
        rc = self.lib.rvcx_dec_margin_frames(ctypes.byref(d), ctypes.byref(m))
        if rc != 0:
            raise _lib.RvcxError(rc, "dec_margin_frames: bad synthesizer configuration")
        return m.value

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
        self.loaded["synth"] = True

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
        d = None if dither is None else self._dev(dither, t.float32).reshape(-1)
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
        d = None if dither is None else self._dev(dither, t.float32).reshape(-1)
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
        if self.fcpe_cfg is None:
            raise _lib.RvcxError(-5, "fcpe weights not loaded (Engine.load_fcpe)")
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
        if self.fcpe_cfg is None:
            raise _lib.RvcxError(-5, "fcpe weights not loaded (Engine.load_fcpe)")
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

    def fcpe_decode(self, salience, threshold: float = 0.006, decoder: str = "local_argmax", interp_uv: bool = False,
                    pad_to=None):
        """rvcx_fcpe_decode: the cents decoder (+ post_process) alone on salience [F][out_dims] -> f0 fp64."""
        if self.fcpe_cfg is None:
            raise _lib.RvcxError(-5, "fcpe weights not loaded (Engine.load_fcpe)")
        t = self.torch
        p = self._dev(salience, t.float32).reshape(-1, self.fcpe_cfg["out_dims"]).contiguous()
        F = int(p.shape[0])
        n_out = int(pad_to) if (interp_uv and pad_to) else F
        f0 = t.empty((n_out,), dtype=t.float64, device=self.device)
        self._check(self.lib.rvcx_fcpe_decode(self.ctx, p.data_ptr(), F, float(threshold),
                                              self._FCPE_DECODERS[decoder], 1 if interp_uv else 0, int(pad_to or 0),
                                              f0.data_ptr(), self.stream()), "fcpe_decode")
        return f0

    def fcpe_mel(self, audio):
        """The FCPE network's input alone (rvcx_fcpe_mel, include/rvcx_test.h): audio [N] -> log-mel [F, num_mels]."""
        if self.fcpe_cfg is None:
            raise _lib.RvcxError(-5, "fcpe weights not loaded (Engine.load_fcpe)")
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        F = self._fcpe_frames(a.numel())
        mel = t.empty((F, self.fcpe_cfg["num_mels"]), dtype=t.float32, device=self.device)
        fo = ctypes.c_int64(0)
        self._check(self.lib.rvcx_fcpe_mel(self.ctx, a.data_ptr(), a.numel(), mel.data_ptr(), F, ctypes.byref(fo),
                                           self.stream()), "fcpe_mel")
        assert fo.value == F, (fo.value, F)
        return mel

    def performer_attention(self, q, k, v, proj):
        """The Performer attention kernels alone (rvcx_performer_attention, include/rvcx_test.h): q, k, v
        [H][T][64], proj [M][64] -> [H][T][64]."""
        t = self.torch
        q, k, v, pm = (self._dev(x, t.float32) for x in (q, k, v, proj))
        H, T, D = (int(x) for x in q.shape)
        if D != 64 or k.shape != q.shape or v.shape != q.shape or pm.shape[1] != 64:
            raise ValueError("performer_attention: q, k, v [H][T][64] and proj [M][64]")
        out = t.empty_like(q)
        self._check(self.lib.rvcx_performer_attention(self.ctx, q.data_ptr(), k.data_ptr(), v.data_ptr(), H, T,
                                                      pm.data_ptr(), int(pm.shape[0]), out.data_ptr(), self.stream()),
                    "performer_attention")
        return out

    def performer_attention_batch(self, q, k, v, proj):
        """rvcx_performer_attention_b (include/rvcx_test.h): q, k, v [B][H][T][64], proj [M][64] -> [B][H][T][64], the
        B streams in one set of launches."""
        t = self.torch
        q, k, v, pm = (self._dev(x, t.float32).contiguous() for x in (q, k, v, proj))
        if q.dim() != 4 or q.shape[3] != 64 or k.shape != q.shape or v.shape != q.shape or pm.shape[1] != 64:
            raise ValueError("performer_attention_batch: q, k, v [B][H][T][64] and proj [M][64]")
        B, H, T, _ = (int(x) for x in q.shape)
        out = t.empty_like(q)
        self._check(self.lib.rvcx_performer_attention_b(self.ctx, q.data_ptr(), k.data_ptr(), v.data_ptr(), B, H, T,
                                                        pm.data_ptr(), int(pm.shape[0]), out.data_ptr(),
                                                        self.stream()), "performer_attention_b")
        return out

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
        rows = [self._dev(a, t.float32).reshape(-1) for a in audios]
        B = len(rows)
        if B < 1:
            return []
        ns = [int(r.numel()) for r in rows]
        lda = max(ns)
        a = t.zeros((B, lda), dtype=t.float32, device=self.device)
        for b, r in enumerate(rows):
            a[b, : ns[b]] = r
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

    def synth_infer(self, phone, lengths, pitch, pitchf, sid, eps_z=None, eps_src=None, seed: int = 0,
                    want_latents: bool = False):
        t = self.torch
        ph = self._dev(phone, t.float32)
        B, T = int(ph.shape[0]), int(ph.shape[1])
        ln = self._dev(lengths, t.int32).reshape(B)
        pc = None if pitch is None else self._dev(pitch, t.int32).reshape(B, T)
        pf = None if pitchf is None else self._dev(pitchf, t.float32).reshape(B, T)
        sd = self._dev(sid, t.int32).reshape(B)
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        I = self.synth_cfg.inter_channels
        zp = t.empty((B, T, I), dtype=t.float32, device=self.device) if want_latents else None
        z = t.empty((B, T, I), dtype=t.float32, device=self.device) if want_latents else None
        self._check(self.lib.rvcx_synth_infer(self.ctx, B, T, ph.data_ptr(), ln.data_ptr(), _ptr(pc),
                                              _ptr(pf), sd.data_ptr(), _ptr(ez), _ptr(es),
                                              ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(), _ptr(zp),
                                              _ptr(z), self.stream()), "synth_infer")
        return (out, zp, z) if want_latents else out

    def synth_infer_ex(self, phone, lengths, pitch, pitchf, sid, rate=None, eps_z=None, eps_src=None, seed: int = 0):
        """Synthesizer.infer with rate and the full return value (rvcx_synth_infer_ex): -> (out [B][T' upp],
        z_p [B][T'][I], z [B][T'][I], m_p [B][T][I], logs_p [B][T][I]) with T' = T - int(T (1 - rate))."""
        t = self.torch
        ph = self._dev(phone, t.float32)
        B, T = int(ph.shape[0]), int(ph.shape[1])
        ln = self._dev(lengths, t.int32).reshape(B)
        pc = None if pitch is None else self._dev(pitch, t.int32).reshape(B, T)
        pf = None if pitchf is None else self._dev(pitchf, t.float32).reshape(B, T)
        sd = self._dev(sid, t.int32).reshape(B)
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        I = self.synth_cfg.inter_channels
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        zp = t.empty((B, T, I), dtype=t.float32, device=self.device)
        z = t.empty((B, T, I), dtype=t.float32, device=self.device)
        mp = t.empty((B, T, I), dtype=t.float32, device=self.device)
        lp = t.empty((B, T, I), dtype=t.float32, device=self.device)
        tn = ctypes.c_int(0)
        self._check(self.lib.rvcx_synth_infer_ex(self.ctx, B, T, ph.data_ptr(), ln.data_ptr(), _ptr(pc), _ptr(pf),
                                                 sd.data_ptr(), -1.0 if rate is None else float(rate), _ptr(ez),
                                                 _ptr(es), ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(),
                                                 zp.data_ptr(), z.data_ptr(), mp.data_ptr(), lp.data_ptr(),
                                                 ctypes.byref(tn), self.stream()), "synth_infer_ex")
        Tn = int(tn.value)
        return (out.reshape(-1)[: B * Tn * self.upp].reshape(B, Tn * self.upp), zp.reshape(-1)[: B * Tn * I].reshape(B, Tn, I),
                z.reshape(-1)[: B * Tn * I].reshape(B, Tn, I), mp, lp)

    def dec_only(self, z, f0, sid, eps_src=None, seed: int = 0):
        t = self.torch
        zz = self._dev(z, t.float32)
        B, I, T = zz.shape
        f = None if f0 is None else self._dev(f0, t.float32).reshape(B, T)
        sd = self._dev(sid, t.int32).reshape(B)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_dec_only(self.ctx, B, T, zz.data_ptr(), _ptr(f), sd.data_ptr(), _ptr(es),
                                           ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(),
                                           self.stream()), "dec_only")
        return out

    def voice_conversion(self, audio_pad, pitch, pitchf, sid: int, protect: float, eps_z=None, eps_src=None,
                         seed: int = 0, index_rate: float = 0.0):
        """HuBERT -> x2 upsample -> protect -> Synthesizer.infer on one padded chunk (device in/out)."""
        t = self.torch
        a = self._dev(audio_pad, t.float32).reshape(-1)
        n = a.numel()
        pc = None if pitch is None else self._dev(pitch, t.int32).reshape(-1)
        pf = None if pitchf is None else self._dev(pitchf, t.float32).reshape(-1)
        cap = (n // 160) * self.upp
        out = t.empty((cap,), dtype=t.float32, device=self.device)
        no = ctypes.c_int64(0)
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        self._check(self.lib.rvcx_voice_conversion(self.ctx, a.data_ptr(), n, _ptr(pc), _ptr(pf), int(sid),
                                                   float(protect), float(index_rate), _ptr(ez), _ptr(es),
                                                   ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(), cap,
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
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        self._check(self.lib.rvcx_pipeline(self.ctx, a.data_ptr(), n, int(sid), float(semitones), float(protect),
                                           int(t_pad), int(t_pad_tgt), _ptr(ez), _ptr(es),
                                           ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(), out.numel(),
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

    def set_generator_precision(self, precision):
        """Removed in round 4: the fp16 streaming generator is a per-hop option (StreamGroup.process(...,
        gen_precision=...), rvcx_rt_opts.gen_precision). Raises RvcxError(RVCX_E_INVALID) with that message."""
        self._check(self.lib.rvcx_set_generator_precision(self.ctx, int(precision)), "set_generator_precision")

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
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        self._check(self.lib.rvcx_pipeline_ex(self.ctx, a.data_ptr(), n, ctypes.byref(opts), _ptr(ez), _ptr(es),
                                              ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(), out.numel(),
                                              ctypes.byref(no), _ptr(f0), self.stream()), "pipeline_ex")
        res = out[: no.value]
        return (res, f0) if want_f0 else res

    def _pipeline_rows(self, a, ns, opts, sids, eps_z, eps_src, seed, out, want_f0, want_hidden):
        """What rvcx_pipeline_batch and rvcx_pipeline_batch_v share: a [B, lda] fp64 on device, rows of ns samples
        (an int: the equal-length entry). Returns (out [B, ldo], n_out per row, f0 [B, F] or None, salience or None)."""
        t = self.torch
        B, lda = int(a.shape[0]), int(a.shape[1])
        m = lda + 2 * int(opts.t_pad)
        ldo = (m // 160) * self.upp
        if out is None or out.numel() < B * ldo:
            out = t.empty((B, ldo), dtype=t.float32, device=self.device)
        out = out.reshape(-1)[: B * ldo].reshape(B, ldo)
        sid = np.broadcast_to(np.asarray(sids, dtype=np.int32), (B,))
        sarr = (ctypes.c_int32 * B)(*[int(v) for v in sid])
        ez = None if eps_z is None else self._dev(eps_z, t.float32)
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        F = 1 + m // 160
        f0 = t.empty((B, F), dtype=t.float64, device=self.device) if want_f0 else None
        hid = t.empty((B, F, 360), dtype=t.float32, device=self.device) if want_hidden else None
        head = (self.ctx, a.data_ptr())
        mid = (lda, B, ctypes.byref(opts), sarr, _ptr(ez), _ptr(es), ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF),
               out.data_ptr(), ldo)
        if isinstance(ns, int):
            no = ctypes.c_int64(0)
            self._check(self.lib.rvcx_pipeline_batch(*head, ns, *mid, ctypes.byref(no), _ptr(f0), _ptr(hid),
                                                     self.stream()), "pipeline_batch")
            return out, [int(no.value)] * B, f0, hid
        no = (ctypes.c_int64 * B)()
        self._check(self.lib.rvcx_pipeline_batch_v(*head, (ctypes.c_int64 * B)(*ns), *mid, no, _ptr(f0), F,
                                                   self.stream()), "pipeline_batch_v")
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
                         want_f0: bool = False):
        """Utterances of different lengths (a list of fp64 [n_b] arrays @16 kHz, each within t_max) through one
        batched pass (rvcx_pipeline_batch_v). Returns a list of fp32 [n_out_b] device tensors (row b =
        Pipeline.pipeline of utterance b); with want_f0 also the list of the rows' adjusted f0 (fp64 [F_b]).
        eps_z [B, inter, T_max] / eps_src [B, T_max * upp] with T_max = max pipeline_frames(n_b): row b consumes
        eps_z[b, :, :T_b] and eps_src[b, :T_b * upp]."""
        t = self.torch
        rows = [self._dev(a, t.float64).reshape(-1) for a in audios]
        B = len(rows)
        if B < 1:
            return ([], []) if want_f0 else []
        ns = [int(r.numel()) for r in rows]
        a = t.zeros((B, max(ns)), dtype=t.float64, device=self.device)
        for b, r in enumerate(rows):
            a[b, : ns[b]] = r
        out, no, f0, _ = self._pipeline_rows(a, ns, opts, sids, eps_z, eps_src, seed, None, want_f0, False)
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

    def rt_model_rows(self, group, rows: int, gated: bool):
        """The model rows [rows, frames * upp] of a StreamGroup's last hop before (gated False) or after the noise
        gate (rvcx_rt_model_rows, include/rvcx_test.h); rows = that hop's active streams."""
        t = self.torch
        n = group.geometry["frames"] * self.upp
        out = t.empty((int(rows), n), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_rt_model_rows(self.ctx, group.handle, 1 if gated else 0, out.data_ptr(), n,
                                                self.stream()), "rt_model_rows")
        return out

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

    def kmeans_assign(self, x, cent, want_dist: bool = True):
        """One nearest-centroid pass (rvcx_kmeans_assign): x [n, d], cent [nlist, d] -> (assign int32 [n],
        dist fp32 [n] or None) device tensors."""
        t = self.torch
        xx, cc = self._dev(x, t.float32), self._dev(cent, t.float32)
        n, d = xx.shape
        assign = t.empty((n,), dtype=t.int32, device=self.device)
        dist = t.empty((n,), dtype=t.float32, device=self.device) if want_dist else None
        self._check(self.lib.rvcx_kmeans_assign(self.ctx, xx.data_ptr(), n, d, cc.data_ptr(), cc.shape[0],
                                                assign.data_ptr(), _ptr(dist), self.stream()), "kmeans_assign")
        return assign, dist

    def kmeans_update(self, x, assign, cent):
        """One centroid update (rvcx_kmeans_update): -> (new centroids fp32 [nlist, d], sizes int64 [nlist])
        device tensors; cent is not modified."""
        t = self.torch
        xx, aa = self._dev(x, t.float32), self._dev(assign, t.int32)
        cc = self._dev(cent, t.float32).clone()
        n, d = xx.shape
        sizes = t.empty((cc.shape[0],), dtype=t.int64, device=self.device)
        self._check(self.lib.rvcx_kmeans_update(self.ctx, xx.data_ptr(), n, d, aa.data_ptr(), cc.shape[0],
                                                cc.data_ptr(), sizes.data_ptr(), self.stream()), "kmeans_update")
        return cc, sizes

    def gru_bidir(self, gi, whh_f, bhh_f, whh_b, bhh_b, tag_start: int = 0):
        """RMVPE's BiGRU recurrence alone (rvcx_gru_bidir, include/rvcx_test.h): gi [B, T, 1536], W_hh [768, 256] and
        b_hh [768] per direction -> out [B, T, 512] (device). tag_start < 0 continues the hand-off tag counters of the
        context's buffer, >= 0 zeroes the buffer and sets them."""
        t = self.torch
        g = self._dev(gi, t.float32)
        B, T, _ = g.shape
        assert g.shape[2] == 1536
        w = [self._dev(x, t.float32) for x in (whh_f, bhh_f, whh_b, bhh_b)]
        assert tuple(w[0].shape) == (768, 256) == tuple(w[2].shape) and w[1].numel() == 768 == w[3].numel()
        out = t.empty((B, T, 512), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_gru_bidir(self.ctx, g.data_ptr(), B, T, w[0].data_ptr(), w[1].data_ptr(),
                                            w[2].data_ptr(), w[3].data_ptr(), out.data_ptr(), int(tag_start),
                                            self.stream()), "gru_bidir")
        return out

    def dec_source(self, f0, eps_src=None, seed: int = 0):
        """The decoder's harmonic source alone (rvcx_dec_source, include/rvcx_test.h): f0 [B, T] -> har
        [B, T * upp] (device), NSF SineGen or the MRF source of the loaded configuration; eps_src as dec_only's."""
        t = self.torch
        f = self._dev(f0, t.float32)
        B, T = f.shape
        es = None if eps_src is None else self._dev(eps_src, t.float32)
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_dec_source(self.ctx, B, T, f.data_ptr(), _ptr(es),
                                             ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), out.data_ptr(), self.stream()),
                    "dec_source")
        return out

    # ------------------------------------------------------------------ kernel timing
    def set_conv_math(self, mode: str):
        """Contraction arithmetic of this context: "h16" (the default: fp32 via three bf16 planes on bf16 MFMA, the
        generator's weight-streamed convs and fused ResBlock pairs via two fp16 planes), "split" (three bf16 planes
        everywhere) or "f32" (fp32-input MFMA) (rvcx_set_conv_math)."""
        m = {"default": 0, "f32": 1, "split": 2, "h16": 3}[mode]
        self._check(self.lib.rvcx_set_conv_math(self.ctx, m), "set_conv_math")
        self.conv_math = m

    def conv1d(self, x, w, bias=None, dilation: int = 1, padding: int = 0, stride: int = 1, math: str = "default"):
        """torch.nn.functional.conv1d(x.T[None], w, bias, stride, padding, dilation)[0].T on the device kernel:
        x [T][C_in] (time-major), w [N][C_in][taps] (torch layout) -> [T_out][N] fp32 (rvcx_conv1d)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C, K = (int(v) for v in w.shape)
        wk = self._dev(w.permute(2, 0, 1).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        T = int(x.shape[0])
        T_out = (T + 2 * padding - dilation * (K - 1) - 1) // stride + 1
        y = torch.empty((T_out, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1, "split": 2, "wsb": 3, "gs": 4, "h16": 5, "f16": 6, "gs_h16": 7}[math]
        self._check(self.lib.rvcx_conv1d(self.ctx, _ptr(x), T, C, _ptr(wk), _ptr(b), N, K, dilation, padding, stride,
                                         m, _ptr(y), T_out, self.stream()), "conv1d")
        return y

    def conv1d_gen(self, x, w, bias=None, dilation: int = 1, padding: int = 0, pre_slope: float = 0.1,
                   slope=None, res=None, acc=None, acc_mode: int = 0, acc_div: float = 1.0,
                   kernel: str = "policy"):
        """The generator's fused conv (rvcx_conv1d_gen): y = acc(act(conv1d(pre(x), w, bias)) + res), pre = leaky
        ReLU(pre_slope) unless pre_slope is None, act = leaky ReLU(slope) unless slope is None, acc_mode 0 store / 1 add
        / 2 add-then-divide into `acc` (the
        initial y); kernel "policy", "wsb" (weight-streamed) or "wst" (weight-stationary). x [T][C_in], w [N][C_in][taps]
        -> [T_out][N] fp32 in the two-plane fp16 split."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C, K = (int(v) for v in w.shape)
        wk = self._dev(w.permute(2, 0, 1).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        r = self._dev(res, torch.float32) if res is not None else None
        T = int(x.shape[0])
        T_out = T + 2 * padding - dilation * (K - 1)
        if acc is not None:
            y = self._dev(acc, torch.float32).clone()
        else:
            y = torch.empty((T_out, N), dtype=torch.float32, device=self.device)
        kn = {"policy": 0, "wsb": 1, "wst": 2}[kernel]
        self._check(self.lib.rvcx_conv1d_gen(self.ctx, _ptr(x), T, C, _ptr(wk), _ptr(b), N, K, dilation, padding,
                                             0 if pre_slope is None else 1,
                                             0.0 if pre_slope is None else float(pre_slope), 0 if slope is None else 1,
                                             0.0 if slope is None else float(slope), _ptr(r), int(acc_mode),
                                             float(acc_div), kn, _ptr(y), self.stream()), "conv1d_gen")
        return y

    ROUTES = {"policy": 0, "f32": 1, "emu": 2, "wsb": 3, "gs": 4, "wst": 5}

    def conv1d_ex(self, x, w, y, *, T_in: int, C_in: int, N: int, T_out: int, ldx: int, ldy: int, taps: int = 1,
                  dil: int = 1, pad: int = 0, stride: int = 1, ldr: int = 0, bias=None, res=None, mask=None,
                  pre_mask=None, batch: int = 1, x_bs: int = 0, y_bs: int = 0, res_bs: int = 0, mask_bs: int = 0,
                  pre_mask_bs: int = 0, batch_inner: int = 1, x_bs2: int = 0, w_bs2: int = 0, y_bs2: int = 0,
                  res_bs2: int = 0, bias_bs2: int = 0, pre_act: int = 0, pre_slope: float = 0.0, act: int = 0,
                  slope: float = 0.0, alpha: float = 1.0, res_mode: int = 0, acc_mode: int = 0, acc_div: float = 1.0,
                  gate_h: int = 0, gate_g=None, gate_g_bs: int = 0, ln_g=None, ln_b=None, ln_eps: float = 1e-5,
                  nz_har=None, nz_bs: int = 0, nz_stride: int = 0, nz_kk: int = 0, nz_u: int = 1, nz_C: int = 0,
                  nz_w=None, nz_b=None, route="policy", no_splitk: bool = False):
        """One 1-D contraction in any form the runtime issues (rvcx_conv1d_ex, include/rvcx.h): the fields of the
        dispatcher's record, strides in floats. Every operand is a float32 tensor on this device and is passed as it
        is -- a view's offset is its base pointer, nothing is copied or made contiguous -- and `y` is written in place.
        Each operand's extent (the last element the form addresses) is checked against the storage behind its tensor
        before the launch (ValueError). Returns (y, kernel family name, planned split count)."""
        torch = self.torch
        G, B, i64 = int(batch_inner), int(batch), int

        def span(t, name, last):
            """`last`: the largest element offset from t's first element that the form addresses."""
            if t is None:
                return None
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device):
                raise ValueError(f"conv1d_ex: {name} must be a float32 tensor on {self.device}")
            room = t.untyped_storage().nbytes() // 4 - t.storage_offset()
            if last < 0 or last >= room:
                raise ValueError(f"conv1d_ex: {name} addresses element {last}, its storage holds {room} from the view")
            return t.data_ptr()

        ncol = gate_h if gate_h > 0 else N
        d = _lib.ConvTestDesc()
        d.x = span(x, "x", (B - 1) * x_bs + (G - 1) * x_bs2 + (T_in - 1) * ldx + C_in - 1)
        d.w = span(w, "w", (G - 1) * w_bs2 + taps * N * C_in - 1)
        d.y = span(y, "y", (B - 1) * y_bs + (G - 1) * y_bs2 + (T_out - 1) * ldy + ncol - 1)
        d.bias = span(bias, "bias", (G - 1) * bias_bs2 + N - 1)
        d.res = span(res, "res", (B - 1) * res_bs + (G - 1) * res_bs2 + (T_out - 1) * ldr + N - 1)
        d.mask = span(mask, "mask", (B - 1) * mask_bs + T_out - 1)
        d.pre_mask = span(pre_mask, "pre_mask", (B - 1) * pre_mask_bs + T_in - 1)
        d.gate_g = span(gate_g, "gate_g", (B - 1) * gate_g_bs + N - 1)
        d.ln_g, d.ln_b = span(ln_g, "ln_g", N - 1), span(ln_b, "ln_b", N - 1)
        d.nz_har = span(nz_har, "nz_har", (B - 1) * nz_bs + (T_out * nz_u - 1) * nz_stride + max(nz_kk, 1) - 1)
        d.nz_w = span(nz_w, "nz_w", nz_C * max(nz_stride, 1) * max(-(-nz_kk // max(nz_stride, 1)), 1) - 1)
        d.nz_b = span(nz_b, "nz_b", nz_C - 1)
        for k, v in dict(T_in=T_in, C_in=C_in, N=N, taps=taps, dil=dil, pad=pad, stride=stride, T_out=T_out, ldx=ldx,
                         ldy=ldy, ldr=ldr, batch=B, x_bs=x_bs, y_bs=y_bs, res_bs=res_bs, mask_bs=mask_bs,
                         pre_mask_bs=pre_mask_bs, batch_inner=G, x_bs2=x_bs2, w_bs2=w_bs2, y_bs2=y_bs2,
                         res_bs2=res_bs2, bias_bs2=bias_bs2, pre_act=pre_act, act=act, res_mode=res_mode,
                         acc_mode=acc_mode, gate_h=gate_h, gate_g_bs=gate_g_bs, nz_bs=nz_bs, nz_stride=nz_stride,
                         nz_kk=nz_kk, nz_u=nz_u, nz_C=nz_C).items():
            setattr(d, k, i64(v))
        d.pre_slope, d.slope, d.alpha, d.acc_div, d.ln_eps = (float(pre_slope), float(slope), float(alpha),
                                                              float(acc_div), float(ln_eps))
        d.route = self.ROUTES[route] if isinstance(route, str) else int(route)
        d.no_splitk = 1 if no_splitk else 0
        self.last_conv_desc = d  # what conv_plan() queries the planner with
        kind, ksplit = ctypes.c_int(-1), ctypes.c_int(0)
        self._check(self.lib.rvcx_conv1d_ex(self.ctx, ctypes.byref(d), ctypes.byref(kind), ctypes.byref(ksplit),
                                            self.stream()), "conv1d_ex")
        name = self.lib.rvcx_profile_kind_name(kind.value)
        return y, (name.decode() if name else "other"), int(ksplit.value)

    def conv_plan(self, desc=None, static_weight: bool = True):
        """What the planner decides under the size policy for a conv1d_ex descriptor (the last one launched unless given)
        in this context's arithmetic: (kernel family name, tile id, split count, weight image format). Host only
        (rvcx_conv_plan, include/rvcx_test.h)."""
        out = [ctypes.c_int(-1) for _ in range(4)]
        d = self.last_conv_desc if desc is None else desc
        self._check(self.lib.rvcx_conv_plan(ctypes.byref(d), None, 0, 1 if static_weight else 0,
                                            getattr(self, "conv_math", 0), 0, -1, -1, *[ctypes.byref(o) for o in out]),
                    "conv_plan")
        name = self.lib.rvcx_profile_kind_name(out[0].value)
        return (name.decode() if name else "other"), out[1].value, out[2].value, out[3].value

    def conv2d3x3(self, x, w, bias=None, relu: bool = False, math: str = "default"):
        """torch.nn.functional.conv2d(x.permute(2, 0, 1)[None], w, bias, padding=1)[0].permute(1, 2, 0) on the device
        kernel: x [H][W][C_in] (NHWC), w [N][C_in][3][3] (torch layout) -> [H][W][N] fp32 (rvcx_conv2d3x3); math
        "default" = the context's arithmetic, "f32" = exact fp32, "gsw" = the U-Net deep levels' windowed kernel in the
        fp16 split (K split over workgroups)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C = int(w.shape[0]), int(w.shape[1])
        wk = self._dev(w.permute(2, 3, 0, 1).reshape(9, N, C).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        H, W = int(x.shape[0]), int(x.shape[1])
        y = torch.empty((H, W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1, "gsw": 2}[math]
        self._check(self.lib.rvcx_conv2d3x3(self.ctx, _ptr(x), H, W, C, _ptr(wk), _ptr(b), N, 1 if relu else 0, m,
                                            _ptr(y), self.stream()), "conv2d3x3")
        return y

    def convtranspose2d_s2(self, x, w, bias=None, relu: bool = False, math: str = "default"):
        """torch.nn.functional.conv_transpose2d(x.permute(2, 0, 1)[None], w, bias, stride=2, padding=1,
        output_padding=1)[0].permute(1, 2, 0) on the device (rvcx_convtranspose2d_s2, the U-Net decoder's up-conv as
        the pipeline runs it): x [H][W][C_in] (NHWC), w [C_in][N][3][3] (torch layout) -> [2H][2W][N] fp32; math
        "default" = the context's arithmetic, "f32" = exact fp32."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        wd = self._dev(torch.as_tensor(w, dtype=torch.float32).contiguous(), torch.float32)
        C, N = int(wd.shape[0]), int(wd.shape[1])
        b = self._dev(bias, torch.float32) if bias is not None else None
        H, W = int(x.shape[0]), int(x.shape[1])
        y = torch.empty((2 * H, 2 * W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1}[math]
        self._check(self.lib.rvcx_convtranspose2d_s2(self.ctx, _ptr(x), H, W, C, _ptr(wd), _ptr(b), N,
                                                     1 if relu else 0, m, _ptr(y), self.stream()), "convtranspose2d_s2")
        return y

    def flash_attention(self, qkv, n_heads: int, qscale: float, rel_k=None, rel_v=None, window: int = 0, mask=None):
        """The fused attention core (rvcx_flash_attention): qkv [B][T][3 H] time-major (q | k | v, heads of dk inside
        each), optional relative tables rel_k / rel_v [2 window + 1][dk] and key/query mask [B][T] -> [B][T][H]."""
        torch = self.torch
        q = self._dev(qkv, torch.float32)
        B, T, H3 = (int(v) for v in q.shape)
        dk = H3 // 3 // n_heads
        rk = None if rel_k is None else self._dev(rel_k, torch.float32)
        rv = None if rel_v is None else self._dev(rel_v, torch.float32)
        mk = None if mask is None else self._dev(mask, torch.float32)
        y = torch.empty((B, T, H3 // 3), dtype=torch.float32, device=self.device)
        self._check(self.lib.rvcx_flash_attention(self.ctx, _ptr(q), B, T, int(n_heads), dk, float(qscale), _ptr(rk),
                                                  _ptr(rv), int(window), _ptr(mk), _ptr(y), self.stream()),
                    "flash_attention")
        return y

    def resblock_pair(self, x, w1, b1, w2, b2, dilation: int, acc=None, acc_mode: int = 0, acc_div: float = 1.0,
                      cfg: int = 0):
        """One ResBlock dilation pair on the fused kernel (rvcx_resblock_pair): x [B][T][C] time-major, w1/w2
        [C][C][k] (torch layout) -> conv2(lrelu(conv1_d(lrelu(x)) + b1)) + b2 + x, stored (acc_mode 0) or
        accumulated into `acc` (1: acc + out, 2: (acc + out) / acc_div)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        B, T, C = (int(v) for v in x.shape)
        k = int(np.shape(w1)[2])
        w1k = self._dev(torch.as_tensor(w1, dtype=torch.float32).permute(2, 0, 1).contiguous(), torch.float32)
        w2k = self._dev(torch.as_tensor(w2, dtype=torch.float32).permute(2, 0, 1).contiguous(), torch.float32)
        b1d, b2d = self._dev(b1, torch.float32), self._dev(b2, torch.float32)
        y = (self._dev(acc, torch.float32).clone() if acc is not None
             else torch.empty((B, T, C), dtype=torch.float32, device=self.device))
        self._check(self.lib.rvcx_resblock_pair(self.ctx, _ptr(x), B, T, C, _ptr(w1k), _ptr(b1d), _ptr(w2k), _ptr(b2d),
                                                k, dilation, acc_mode, float(acc_div), cfg, _ptr(y), self.stream()),
                    "resblock_pair")
        return y

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
