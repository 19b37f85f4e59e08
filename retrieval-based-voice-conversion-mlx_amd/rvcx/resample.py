"""scipy.signal.resample_poly's quantities for the device resampler (rvcx_resample_poly_v, include/rvcx.h).

The filter is designed on the host with scipy, as the pipeline's high-pass is; the device applies it. With up / down
reduced by their gcd, M = max(up, down) and half = 10 M:

    h            = firwin(2 half + 1, 1 / M, window=("kaiser", 5.0)) * up
    n_pre_pad    = down - half % down
    n_pre_remove = (half + n_pre_pad) // down
    n_out        = ceil(n up / down)
    y[j]         = sum_i x[i] h[c - i up],   c = (j + n_pre_remove) down - n_pre_pad,   0 <= c - i up < len(h)
"""
from __future__ import annotations

from functools import lru_cache
from math import gcd
from typing import Tuple

import numpy as np


def reduce(up: int, down: int) -> Tuple[int, int]:
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"up and down must be positive, got {up}/{down}")
    g = gcd(up, down)
    return up // g, down // g


def plan(n: int, up: int, down: int) -> Tuple[int, int, int, int, int]:
    """-> (up, down, n_out, n_pre_pad, n_pre_remove) of resample_poly(x [n], up, down), up / down reduced."""
    up, down = reduce(up, down)
    half = 0 if up == down == 1 else 10 * max(up, down)
    n_pre_pad = down - half % down
    return up, down, -(-int(n) * up // down), n_pre_pad, (half + n_pre_pad) // down


@lru_cache(maxsize=None)
def _taps(up: int, down: int) -> np.ndarray:
    from scipy.signal import firwin

    if up == down == 1:
        h = np.ones(1, dtype=np.float64)
    else:
        m = max(up, down)
        h = np.asarray(firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)), dtype=np.float64) * up
    h.setflags(write=False)
    return h


def taps(up: int, down: int) -> np.ndarray:
    """resample_poly's default filter for up / down (read-only fp64, cached per reduced pair); [1.0] for 1 / 1."""
    return _taps(*reduce(up, down))
