"""The bars of tests/test_gpu_synth_configs.py (K x the oracle's own fp32-vs-fp64 gap, tests/parity_anchor.py) see the
mistakes a runtime can make with a configuration other than SYNTH_48K_V2, and the generator's margin formula
(rvcx_dec_margin_frames) covers the receptive field of every configuration. No GPU.

Mutations of the fp32 oracle at the GPU file's point (lengths (24, 17, 1), seed 7), waveform distance to float64 in
units of the gap (1.0 is the undisturbed oracle), measured on the CPU:

    v2_40k   stage-0 ConvTranspose padding 4 for 3 (a one-sample shift)                             2.3e5
    v2_40k   stage-0 kernel taps 10..15 zeroed (the second live tap of phases 0..2 and 7..9 dropped)  1.7e5
    v1_32k   stage-1 kernel taps 8..15 zeroed (a 3-tap packing of the 5-tap layer)                  4.7e4
    v2_32k   noise_convs.0 padding 17 for 16                                                        5.7e3
    v1_48k   conv_post.weight's 16 channels rolled by one (a 32-channel weight layout read at 16)   4.5e5

Each prints its ratio; all are required beyond K = 8, and the latents (which none of them touches) within 2.

The margin: measured reach / rvcx_dec_margin_frames, in frames: 48 kHz v2 10 / 10, v2_40k 11 / 12, v2_32k 11 / 12,
v1_48k 12 / 13, v1_32k 13 / 14.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_anchor as pa
from parity_anchor import K, PatchedF, anchor, ratios
from synth_configs import CONFIGS, NAMES, margin_frames, weights_for

LENGTHS, SEED = (24, 17, 1), 7

_ANC = {}


def point(name):
    """(case, fn, anchor) of configuration `name` at the GPU file's point, computed once."""
    if name not in _ANC:
        cfg = CONFIGS[name]
        c = pa.synth_case(LENGTHS, SEED, cfg=cfg)
        fn = pa.synth_fn(weights_for(name), cfg=cfg, **c)
        _ANC[name] = (c, fn, anchor(fn))
    return _ANC[name]


def mutated_weights(name, key, edit):
    """A copy of the configuration's state dict with `edit` applied to a copy of w[key]."""
    w = dict(weights_for(name))
    v = np.array(w[key], copy=True)
    edit(v)
    w[key] = v
    return w


def waveform_ratio(name, w=None, over=None, monkeypatch=None):
    from oracle import synth as osynth

    cfg = CONFIGS[name]
    c, fn, anc = point(name)
    base = ratios(fn, anc)
    assert max(base.values()) <= 2.0, base  # the undisturbed fp32 oracle, any summation order
    if w is not None:
        fn = pa.synth_fn(w, cfg=cfg, **c)
    if over is not None:
        monkeypatch.setattr(osynth, "F", PatchedF(**over))
    try:
        r = ratios(fn, anc)
    finally:
        if over is not None:
            monkeypatch.setattr(osynth, "F", F)
    assert max(r[k] for k in ("z_p", "z", "m_p", "logs_p")) <= 2.0, r  # the mutation sits in the generator
    return r["o"]


def test_v2_40k_stage0_padding_shift(monkeypatch):
    """k = 16, u = 10: padding (k - u) / 2 = 3. With 4 (and output_padding 2 to keep T u samples) the stage's output
    is the right one moved by one sample."""
    def ct(x, w, b, stride, padding, output_padding=0):
        if stride == 10 and tuple(w.shape) == (512, 256, 16):
            assert padding == 3 and output_padding == 0
            padding, output_padding = 4, 2
        return F.conv_transpose1d(x, w, b, stride=stride, padding=padding, output_padding=output_padding)

    r = waveform_ratio("v2_40k", over=dict(conv_transpose1d=ct), monkeypatch=monkeypatch)
    print(f"\nv2_40k stage-0 padding 4: {r:.3g} x gap")
    assert r > K, r


def test_v2_40k_stage0_second_tap_dropped():
    """Output phase r reads kernel taps r + 3 (mod 10): phases 0..2 read taps 3..5 and 13..15, phases 7..9 taps 0..2
    and 10..12. Zeroing taps 10..15 drops the second live tap of each."""
    def edit(v):
        assert v.shape == (512, 256, 16)
        v[:, :, 10:] = 0.0

    r = waveform_ratio("v2_40k", w=mutated_weights("v2_40k", "dec.ups.0.weight", edit))
    print(f"\nv2_40k stage-0 taps 10..15 zeroed: {r:.3g} x gap")
    assert r > K, r


def test_v1_32k_stage1_three_tap_packing():
    """u = 4, k = 16, p = 6: five polyphase taps. A packing that keeps three loses kernel taps beyond 2 u."""
    def edit(v):
        assert v.shape == (256, 128, 16)
        v[:, :, 8:] = 0.0

    r = waveform_ratio("v1_32k", w=mutated_weights("v1_32k", "dec.ups.1.weight", edit))
    print(f"\nv1_32k stage-1 taps 8..15 zeroed: {r:.3g} x gap")
    assert r > K, r


def test_v2_32k_noise_conv0_padding(monkeypatch):
    """noise_convs.0 at 32 kHz: stride 8 x 2 x 2 = 32, kernel 64, padding 16; 17 keeps the length (10 T rows)."""
    def c1(x, w, b=None, stride=1, padding=0, dilation=1):
        if stride == 32 and tuple(w.shape) == (256, 1, 64):
            assert padding == 16
            padding = 17
        return F.conv1d(x, w, b, stride=stride, padding=padding, dilation=dilation)

    r = waveform_ratio("v2_32k", over=dict(conv1d=c1), monkeypatch=monkeypatch)
    print(f"\nv2_32k noise_convs.0 padding 17: {r:.3g} x gap")
    assert r > K, r


def test_v1_48k_conv_post_channel_layout():
    """Five stages end at 512 >> 5 = 16 channels; a conv_post (or last ResBlock stage) that reads its weight in a
    layout made for 32 pairs channels with other weights: modelled as the 16 channels of conv_post.weight rolled."""
    def edit(v):
        assert v.shape == (1, 16, 7)
        v[:] = np.roll(v, 1, axis=1)

    r = waveform_ratio("v1_48k", w=mutated_weights("v1_48k", "dec.conv_post.weight", edit))
    print(f"\nv1_48k conv_post channels rolled: {r:.3g} x gap")
    assert r > K, r


# ----------------------------------------------------------------- the receptive-field formula
def reach_frames(cfg, w, T=64, at=32):
    """The generator's measured one-sided reach in frames on the float64 oracle: z perturbed at frame `at` (every
    channel, f0 and the source noise fixed), the farthest output sample that changes, as the distance between its
    frame and `at`."""
    from oracle import synth as osynth

    rng = np.random.Generator(np.random.PCG64(90))
    z = torch.from_numpy(rng.standard_normal((1, cfg.inter_channels, T)))
    f0 = torch.full((1, T), 220.0, dtype=torch.float64)
    es = torch.from_numpy(rng.standard_normal((1, T * cfg.upp)))
    sid = torch.zeros(1, dtype=torch.int64)
    w64 = pa.weights(w, torch.float64)
    a = osynth.dec_only(w64, cfg, z, f0, sid, es).reshape(-1)
    z2 = z.clone()
    z2[:, :, at] += 1.0
    b = osynth.dec_only(w64, cfg, z2, f0, sid, es).reshape(-1)
    idx = torch.nonzero(a != b).reshape(-1)
    lo, hi = int(idx.min()) // cfg.upp, int(idx.max()) // cfg.upp
    assert 0 < lo and hi < T - 1, (lo, hi)  # the reach ends inside the sequence
    return max(at - lo, hi - at)


@pytest.mark.parametrize("name", ("48k_v2",) + NAMES)
def test_margin_covers_measured_reach(synth_w, name):
    """rvcx_dec_margin_frames(cfg) >= the measured reach (the output window keeps enough) and <= reach + 2 (the
    formula's ceilings, one per stage group, do not pile up); the documented 10 for SYNTH_48K_V2."""
    from rvcx.config import SYNTH_48K_V2

    cfg, w = (SYNTH_48K_V2, synth_w) if name == "48k_v2" else (CONFIGS[name], weights_for(name))
    M, reach = margin_frames(cfg), reach_frames(cfg, w)
    print(f"\n{name}: margin {M} frames, measured reach {reach}")
    if name == "48k_v2":
        assert M == 10
    assert reach <= M <= reach + 2, (M, reach)
