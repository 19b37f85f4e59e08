"""What the resampler tests share: the rate pairs, the closed form of scipy.signal.resample_poly in numpy float64 and
the derived error bound.

Closed form (include/rvcx.h, rvcx_resample_poly_v), h of L taps, up / down coprime:
    y[j] = sum_i x[i] h[c - i up],  c = (j + n_pre_remove) down - n_pre_pad,  0 <= i < n,  0 <= c - i up < L

The bound: the device and scipy each sum at most K = ceil(L / up) fp64 products per output, in their own order. A sum
of K products of fp64 numbers computed in any order is within gamma(K + 1) * sum|x h| of the exact value (Higham,
Accuracy and Stability, eq. 3.5: K - 1 additions and one rounding per product; K + 1 covers it with room), so two
such sums differ by at most 2 (K + 1) 2^-53 sum_i |x[i] h[c - i up]|, the sum taken here in float64.
"""
import numpy as np

# (name, rate_in, rate_out): the reduced ratios are 1/3, 160/441, 320/441, 2/1, 3/2, 441/400, 147/160, 441/160
GPU_PAIRS = (("48k_16k", 48000, 16000), ("44k1_16k", 44100, 16000), ("22k05_16k", 22050, 16000),
             ("8k_16k", 8000, 16000), ("32k_48k", 32000, 48000), ("40k_44k1", 40000, 44100),
             ("48k_44k1", 48000, 44100))
CPU_PAIRS = (("48k_16k", 48000, 16000), ("44k1_16k", 44100, 16000), ("16k_44k1", 16000, 44100),
             ("22k05_16k", 22050, 16000), ("40k_44k1", 40000, 44100), ("32k_48k", 32000, 48000))


def closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out):
    """-> (y [n_out], sum_i |x[i] h[c - i up]| [n_out]) in float64; up / down reduced."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, L = len(x), len(h)
    K = -(-L // up)
    j = np.arange(n_out, dtype=np.int64)
    c = (j + n_pre_remove) * down - n_pre_pad
    ih = c // up
    k = np.arange(K - 1, -1, -1, dtype=np.int64)  # ascending input index
    i = ih[:, None] - k[None, :]
    t = (c - ih * up)[:, None] + k[None, :] * up
    ok = (i >= 0) & (i < n) & (t < L)
    prod = np.where(ok, x[np.clip(i, 0, n - 1)] * h[np.clip(t, 0, L - 1)], 0.0)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def bound(absum, L, up):
    """2 (K + 1) 2^-53 sum|x h| per output sample."""
    K = -(-L // up)
    return 2.0 * (K + 1) * 2.0 ** -53 * absum


def worst_ratio(got, ref, bnd):
    """max over the samples of |got - ref| / bound, with 0 / 0 = 0 and anything / 0 = inf."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0


def parent_load_audio(file_path, sr=16000):
    """The host loader as it stood before the device route existed (the five lines of rvcx.infer.infer.load_audio)."""
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
