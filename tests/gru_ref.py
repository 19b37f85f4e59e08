"""A plain bidirectional GRU recurrence given the input projections (test helper, no GPU needed): the reference of
tests/test_gpu_gru.py for csrc/gru.hip.

Cell order as ATen's GRUCell, which the kernel follows (gru.hip:19-20):
    r = sig(hg_r + ig_r), z = sig(hg_z + ig_z), n = tanh(ig_n + hg_n * r), h' = (h - n) * z + n, hg = W_hh h + b_hh.
gi [B, T, 1536] holds x W_ih^T + b_ih, the forward direction's r, z, n (3 x 256) then the backward direction's; the
output [B, T, 512] the forward h then the backward h of every step (the backward direction walks t = T - 1 .. 0 from
h = 0 and writes its state at t). Everything runs in `dtype`.

The perturbed form models activations that are not correctly rounded: every sigmoid value is multiplied by
(1 + u a_s) and every tanh value gets u a_t added, u ~ U(-1, 1) from a seeded generator, drawn anew for every element.
"""
from __future__ import annotations

import numpy as np

H = 256


def gru_direction(gi, whh, bhh, dtype, reverse=False, a_s=0.0, a_t=0.0, rng=None):
    """One direction. gi [B, T, 768] (r, z, n), whh [768, 256], bhh [768] -> h [B, T, 256]."""
    gi = np.asarray(gi).astype(dtype)
    wt = np.ascontiguousarray(np.asarray(whh).astype(dtype).T)
    bhh = np.asarray(bhh).astype(dtype)
    B, T, _ = gi.shape
    h = np.zeros((B, H), dtype)
    out = np.zeros((B, T, H), dtype)
    one = dtype(1)
    pert = a_s != 0.0 or a_t != 0.0
    for s in range(T):
        t = T - 1 - s if reverse else s
        hg = h @ wt + bhh
        ig = gi[:, t]
        r = one / (one + np.exp(-(hg[:, :H] + ig[:, :H])))
        z = one / (one + np.exp(-(hg[:, H:2 * H] + ig[:, H:2 * H])))
        if pert:
            r = (r * (1.0 + a_s * rng.uniform(-1.0, 1.0, r.shape))).astype(dtype)
            z = (z * (1.0 + a_s * rng.uniform(-1.0, 1.0, z.shape))).astype(dtype)
        n = np.tanh(ig[:, 2 * H:] + hg[:, 2 * H:] * r)
        if pert:
            n = (n + a_t * rng.uniform(-1.0, 1.0, n.shape)).astype(dtype)
        h = ((h - n) * z + n).astype(dtype)
        out[:, t] = h
    return out


def gru_bidir(gi, whh_f, bhh_f, whh_b, bhh_b, dtype=np.float64, a_s=0.0, a_t=0.0, seed=0):
    """gi [B, T, 1536] (or [T, 1536]) -> [B, T, 512] (or [T, 512]) in `dtype`; a_s / a_t: the perturbation amplitudes
    of the sigmoids (relative) and the tanh (absolute), drawn from default_rng(seed)."""
    dtype = np.dtype(dtype).type
    gi = np.asarray(gi)
    single = gi.ndim == 2
    g = gi[None] if single else gi
    assert g.ndim == 3 and g.shape[2] == 6 * H, g.shape
    rng = np.random.default_rng(seed) if (a_s != 0.0 or a_t != 0.0) else None
    f = gru_direction(g[:, :, :3 * H], whh_f, bhh_f, dtype, False, a_s, a_t, rng)
    b = gru_direction(g[:, :, 3 * H:], whh_b, bhh_b, dtype, True, a_s, a_t, rng)
    out = np.concatenate([f, b], axis=2)
    return out[0] if single else out
