"""The realtime noise gate restated with torch (test helper, no GPU needed).

rvc/realtime/core.py:86-94 builds noisereduce.torchgate.TorchGate(tgt_sr, prop_decrease=clean_strength) and
rvc/realtime/pipeline.py:326-327 applies it to every hop's model output. This is that module's stationary mode
without a separate noise clip, written over torch.stft / torch.istft / conv2d so that the STFT conventions are torch's
own; run in float64 it is the answer the device kernels (csrc/spectral_gate.hip) are held to. noisereduce itself is
not a dependency of the tests: the restatement is unpinned against noisereduce's own run.
"""
from __future__ import annotations

import numpy as np
import torch

N_FFT = 1024
HOP = 256
BINS = N_FFT // 2 + 1
EPS = 2.220446049250313e-16  # torch.finfo(torch.float64).eps, added to |X| before the log
TOP_DB = 40.0
N_STD = 1.5


def filter_sizes(sr: int):
    """(n_f, n_t): half widths of the smoothing filter, 500 Hz and 50 ms, as Python's double arithmetic gives them."""
    return int(500 / (sr / (N_FFT / 2))), int(50 / ((HOP / sr) * 1000))


def n_out(n: int) -> int:
    """Samples torch.istft returns without `length`: hop * (frames - 1), frames = 1 + n // hop."""
    return HOP * (n // HOP)


def frames(n: int) -> int:
    return 1 + n // HOP


def smoothing_filter(sr: int, dtype):
    """outer(v_f, v_t) / sum: [1, 1, 2 n_f + 1, 2 n_t + 1]."""
    n_f, n_t = filter_sizes(sr)

    def tri(m):
        return torch.cat([torch.arange(1, m + 1, dtype=dtype) / (m + 1), torch.ones(1, dtype=dtype),
                          torch.arange(m, 0, -1, dtype=dtype) / (m + 1)])

    k = torch.outer(tri(n_f), tri(n_t))
    return (k / k.sum())[None, None]


def gate(x, sr: int, p: float, dtype, mask=None):
    """x [B, n] -> (y [B, n_out(n)], margin [B, 513, F], mask [B, 513, F] bool). margin = X_db - thresh; a given
    `mask` replaces the comparison margin > 0."""
    x = (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(dtype)
    win = torch.hann_window(N_FFT, periodic=True, dtype=dtype)
    X = torch.stft(x, N_FFT, HOP, N_FFT, win, center=True, pad_mode="constant", return_complex=True)
    X_db = 20 * torch.log10(X.abs() + EPS)
    X_db = torch.max(X_db, X_db.max(dim=2, keepdim=True).values - TOP_DB)
    thresh = X_db.mean(dim=2, keepdim=True) + N_STD * X_db.std(dim=2, keepdim=True)
    margin = X_db - thresh
    if mask is None:
        mask = margin > 0
    mask = (mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.asarray(mask))).to(torch.bool)
    s = p * (mask.to(dtype) - 1) + 1
    s = torch.nn.functional.conv2d(s[:, None], smoothing_filter(sr, dtype), padding="same")[:, 0]
    y = torch.istft(X * s, N_FFT, HOP, N_FFT, win, center=True)
    return y, margin, mask


def gate_rows(n: int, seed: int = 3):
    """The gate tests' two rows at 48 kHz (PCG64(seed)): A a 220 Hz tone switched at 3 Hz over a noise floor, B noise
    with a linear ramp. float32 [2, n]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / 48000.0
    a = 0.3 * np.sin(2 * np.pi * 220 * t) * (np.sin(2 * np.pi * 3 * t) > 0) + 0.01 * rng.standard_normal(n)
    b = 0.5 * rng.standard_normal(n) * np.linspace(0, 1, n)
    return np.stack([a, b]).astype(np.float32)
