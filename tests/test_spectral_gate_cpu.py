"""Host-only checks of the noise gate: the torch restatement (tests/spectral_gate_ref.py) has the filter sizes and
output length the reference's TorchGate has, does at strength 0 what the smoothing's zero padding leaves of the
identity, and puts few enough bins near the
threshold on the GPU test's inputs for the mask comparison there to mean something; the C ABI and the Python surface
carry the new option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spectral_gate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sr, n, seed of the rows) of every gated case of tests/test_gpu_spectral_gate.py
GPU_CASES = [(48000, 2048, 3), (48000, 4100, 3), (48000, 41760, 3), (40000, 4100, 3), (32000, 4100, 3)]
BAND_SHARE = 0.01  # the share of a non-silent row's bins that may lie within delta of the threshold


def test_filter_sizes():
    assert ref.filter_sizes(48000) == (5, 9)
    assert ref.filter_sizes(40000) == (6, 7)
    assert ref.filter_sizes(32000) == (8, 6)
    for sr, shape in ((48000, (11, 19)), (40000, (13, 15)), (32000, (17, 13))):
        k = ref.smoothing_filter(sr, torch.float64)
        assert tuple(k.shape) == (1, 1) + shape
        assert abs(float(k.sum()) - 1.0) < 1e-14
        # separable: the outer product of the two normalised triangles
        n_f, n_t = ref.filter_sizes(sr)
        vf = (n_f + 1 - np.abs(np.arange(-n_f, n_f + 1))) / (n_f + 1) ** 2
        vt = (n_t + 1 - np.abs(np.arange(-n_t, n_t + 1))) / (n_t + 1) ** 2
        np.testing.assert_allclose(k[0, 0].numpy(), np.outer(vf, vt), rtol=0, atol=1e-16)


@pytest.mark.parametrize("n,want", [(2048, 2048), (4100, 4096), (41760, 41728), (2047 + 256, 2048)])
def test_n_out(n, want):
    assert ref.n_out(n) == want
    x = torch.from_numpy(ref.gate_rows(n))
    y, margin, mask = ref.gate(x, 48000, 0.5, torch.float32)
    assert y.shape == (2, want)
    assert margin.shape == mask.shape == (2, 513, ref.frames(n))


def _edge_profile(n_bins, half):
    """conv(ones, normalised triangle of half width `half`, zeros outside) in closed form: the taps that fall inside."""
    w = (half + 1 - np.abs(np.arange(-half, half + 1))) / (half + 1) ** 2
    i = np.arange(n_bins)[:, None] + np.arange(-half, half + 1)[None]
    return (w[None] * ((i >= 0) & (i < n_bins))).sum(axis=1)


def test_strength_zero():
    """p = 0 makes s = 1 before the smoothing, but the smoothing pads with zeros, so s falls below 1 in the outer
    n_f bins and n_t frames of the image: the gate is the identity only for what lies inside them. (On the GPU test's
    rows, which have energy in the lowest bins, p = 0 moves samples by up to 0.67; measured with this restatement in
    float32 and float64 alike.) Two statements that do hold, both to fp32 rounding -- 32 ulp of the largest sample:
    two 10-stage transforms plus the window and the overlap-add:
    a tone centred on bin 100 comes back unchanged on the samples no edge frame reaches, and the test rows come back
    as istft(X * edge) with the edge profile computed in closed form, not by conv2d."""
    n, sr = 8192, 48000
    n_f, n_t = ref.filter_sizes(sr)
    tone = (0.4 * np.sin(2 * np.pi * 100 * np.arange(n) / 1024 + 0.3)).astype(np.float32)[None]
    y, _, _ = ref.gate(tone, sr, 0.0, torch.float32)
    assert y.shape == (1, ref.n_out(n))
    # frame t covers samples [256 t - 512, 256 t + 512); frames n_t .. F - 1 - n_t carry s = 1 in time, and the
    # first two and last two frames see the zero padding (broadband leakage): keep clear of both
    F = ref.frames(n)
    lo, hi = 256 * (n_t - 1) + 512, 256 * (F - n_t) - 512
    assert hi - lo >= 1024
    err = float((y[0, lo:hi] - torch.from_numpy(tone[0, lo:hi])).abs().max())
    print(f"\ntone: max |y - x| on [{lo}, {hi}) = {err:.3e}")
    assert err <= 32 * 2.0 ** -23 * 0.4
    x = ref.gate_rows(4100)
    y, _, _ = ref.gate(x, sr, 0.0, torch.float32)
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    X = torch.stft(torch.from_numpy(x).double(), 1024, 256, 1024, win, center=True, pad_mode="constant",
                   return_complex=True)
    edge = np.outer(_edge_profile(513, n_f), _edge_profile(ref.frames(4100), n_t))
    want = torch.istft(X * torch.from_numpy(edge), 1024, 256, 1024, win, center=True)
    err = float((y.double() - want).abs().max())
    print(f"rows: max |gate(p = 0) - istft(X edge)| = {err:.3e}")
    assert err <= 32 * 2.0 ** -23 * float(np.abs(x).max())


def test_band_condition_on_the_gpu_inputs():
    """At most 1 % of the bins of a non-silent row lie within delta = 8 max |margin32 - margin64| of the threshold."""
    from parity_anchor import anchor

    for sr, n, seed in GPU_CASES:
        x = ref.gate_rows(n, seed)
        a = anchor(lambda dt: ref.gate(x, sr, 0.5, dt)[1])
        m64, gap = a["out"]
        delta = 8 * gap
        share = (np.abs(m64) <= delta).reshape(2, -1).mean(axis=1)
        print(f"\nsr {sr} n {n}: gap_m {gap:.3e} delta {delta:.3e} share in band {share}")
        assert (share <= BAND_SHARE).all(), (sr, n, share)


def test_abi_and_python_surface():
    from rvcx import _lib
    from rvcx.realtime import StreamGroup, VoiceChanger, check_clean_strength
    import inspect

    lib = _lib.load()
    assert {"rvcx_spectral_gate", "rvcx_rt_set_clean", "rvcx_rt_model_rows"} <= set(_lib.exported_symbols())
    # the gate's switch is a setting of the slot (rvcx_rt_set_clean): the hop options struct keeps its 72 bytes
    assert ctypes.sizeof(_lib.RtOpts) == 72 and "clean_audio" not in dict(_lib.RtOpts._fields_)
    vp = ctypes.c_void_p
    assert lib.rvcx_rt_set_clean.argtypes == [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    with open(os.path.join(ROOT, "include", "rvcx.h")) as f:
        h = re.sub(r"\s+", " ", f.read())
    assert ("int rvcx_spectral_gate(rvcx_ctx* ctx, const float* d_x, int B, int64_t n, int64_t ldx, int sr, "
            "const float* strength, float* d_y, int64_t ldy, uint8_t* d_mask, void* stream);") in h
    assert ("int rvcx_rt_set_clean(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, int clean_audio, "
            "double clean_strength);") in h
    # null arguments are refused before any device is touched
    assert lib.rvcx_spectral_gate(None, None, 1, 4096, 4096, 48000, None, None, 4096, None, None) != 0
    assert lib.rvcx_rt_model_rows(None, None, 0, None, 0, None) != 0
    assert lib.rvcx_rt_set_clean(None, None, 0, 1, 0.5) != 0
    for cls in (StreamGroup, VoiceChanger):
        p = inspect.signature(cls.__init__).parameters
        assert p["clean_audio"].default is False and p["clean_strength"].default == 0.5
    p = inspect.signature(StreamGroup.opts).parameters
    assert p["clean_audio"].default is None and p["clean_strength"].default is None
    assert check_clean_strength(0) == 0.0 and check_clean_strength(1) == 1.0
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            check_clean_strength(bad)
    # the options that would otherwise vanish are refused by name, before an engine is looked at
    for name in ("post_process", "vad_enabled"):
        with pytest.raises(ValueError, match=name):
            VoiceChanger(96, 0.1, 0.5, engine=None, **{name: True})
    with pytest.raises(ValueError, match="Engine"):  # an unknown keyword is still accepted: the next check speaks
        VoiceChanger(96, 0.1, 0.5, engine=None, model_path="x.pth", vad_sensitivity=3)
