"""Shows, without a GPU, that the bars RefineGAN is held to see the mistakes such a decoder makes.

  1. Kernel level (tests/refinegan_ref.py, the bounds tests/test_gpu_refinegan_kernels.py asserts): a float32 numpy
     restatement of each kernel of csrc/refinegan.hip sits within its bound; a dropped edge tap, a clamp one row off, a
     wrong half-pixel offset, align_corners, a clamp missing at either end, and a noise block read as [B][T][C] land
     beyond it.
  2. Module level (tests/test_gpu_refinegan.py): on the Synthesizer.infer case of lengths (24, 17, 1) each deviation of
     the decoder, applied to the oracle in float64 by monkeypatching (oracle/ is not edited), must land above K = 8 gaps
     of the float64 waveform. The table is printed; a deviation the bar cannot resolve stays in the table, marked.
"""
import numpy as np
import pytest
import torch

import parity_anchor as pa
import refinegan_ref as rr
from parity_anchor import K, anchor


# ----------------------------------------------------------------- 1. the kernels' bounds
def _resample32(x, ker, orig, width, drop=None, shift=0):
    """k_resample_dw in float32 numpy (an fma chain per output; numpy rounds the product, which the bound covers)."""
    B, T, C = x.shape
    Kt = len(ker)
    T_out = -(-T // orig)
    y = np.zeros((B, T_out, C), np.float32)
    for t in range(T_out):
        r0 = t * orig - width + shift
        acc = np.zeros((B, C), np.float32)
        for k in range(max(-r0, 0), min(Kt, T - r0)):
            if k == drop:
                continue
            acc = (acc + x[:, r0 + k] * ker[k]).astype(np.float32)
        y[:, t] = acc
    return y


@pytest.mark.parametrize("orig,width", rr.UNIT_TAPS[:2])
def test_resample_bound_sees_a_dropped_edge_tap_and_a_shifted_window(orig, width):
    Kt = 2 * width + orig
    rng = np.random.Generator(np.random.PCG64(orig))
    ker = rng.standard_normal(Kt).astype(np.float32)
    ker[[0, -1]] = 1.0
    for T in rr.resample_lengths(orig, width):
        x = rng.standard_normal((2, T, 16)).astype(np.float32)
        ref, bound = rr.resample_ref(x, ker, orig, width)
        assert rr.ratio(_resample32(x, ker, orig, width), ref, bound) <= 1.0
        if T >= Kt:  # both edge taps land inside the input
            assert rr.ratio(_resample32(x, ker, orig, width, drop=0), ref, bound) > 100
            assert rr.ratio(_resample32(x, ker, orig, width, drop=Kt - 1), ref, bound) > 100
        assert rr.ratio(_resample32(x, ker, orig, width, shift=1), ref, bound) > 100
    # the decoder's own taps hide a dropped edge tap: ~1e-6 of the centre tap (why the random unit taps are there)
    real, w = rr.real_taps(2)
    assert abs(real[0]) < 1e-5 * np.abs(real).max()


def _lerp32(x, rate, slope=0.2, offset=0.5, clamp_lo=True, clamp_hi=True):
    """k_lerp_up_cat's interpolated columns in float32 numpy."""
    B, T, C = x.shape
    a = np.where(x > 0, x, x * np.float32(slope)).astype(np.float32)
    t = np.arange(T * rate, dtype=np.float32)
    src = np.float32(1.0 / rate) * (t + np.float32(offset)) - np.float32(offset)
    if clamp_lo:
        src = np.maximum(src, np.float32(0))
    i0 = np.clip(np.floor(src).astype(np.int64), 0, T - 1)
    i1 = np.minimum(i0 + 1, T - 1) if clamp_hi else (i0 + 1) % T
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return (l0[None, :, None] * a[:, i0] + l1[None, :, None] * a[:, i1]).astype(np.float32)


@pytest.mark.parametrize("rate", rr.RATES)
def test_lerp_bound_sees_offset_clamps_and_align_corners(rate):
    rng = np.random.Generator(np.random.PCG64(rate))
    for T in (2, 37):
        x = rng.standard_normal((2, T, 32)).astype(np.float32)
        skip = np.zeros((2, T * rate, 8), np.float32)
        ref, bound = rr.lerp_ref(x, skip, rate)
        ref = ref[..., :32]
        assert rr.ratio(_lerp32(x, rate), ref, bound) <= 1.0
        assert rr.ratio(_lerp32(x, rate, offset=0.0), ref, bound) > 1e3       # no half-pixel offset
        assert rr.ratio(_lerp32(x, rate, clamp_lo=False), ref, bound) > 1e3   # extrapolates before row 0
        assert rr.ratio(_lerp32(x, rate, clamp_hi=False), ref, bound) > 1e3   # reads past the last row
        ac = rr.lerp_ref(x, skip, rate, align_corners=True)[0][..., :32]
        assert rr.ratio(ac, ref, bound) > 1e3


def test_adain_bound_sees_a_transposed_noise_read_and_a_wrong_mode():
    rng = np.random.Generator(np.random.PCG64(3))
    for B, T, C in ((2, 37, 32), (2, 5, 256)):
        x, y0 = (rng.standard_normal((B, T, C)).astype(np.float32) for _ in range(2))
        w = rng.standard_normal(C).astype(np.float32)
        eps = rng.standard_normal((B, C, T)).astype(np.float32)
        for mode in (0, 1, 2):
            ref, bound = rr.adain_ref(x, w, eps, y0, mode)
            v = x + eps.transpose(0, 2, 1) * w
            v = np.where(v > 0, v, v * np.float32(0.2)).astype(np.float32)
            got = v if mode == 0 else (y0 + v if mode == 1 else ((y0 + v) / np.float32(3)).astype(np.float32))
            assert rr.ratio(got, ref, bound) <= 1.0
            wrong = rr.adain_ref(x, w, eps.reshape(B, T, C).transpose(0, 2, 1), y0, mode)[0]  # read as [B][T][C]
            assert rr.ratio(wrong, ref, bound) > 1e3
            assert rr.ratio(rr.adain_ref(x, w, eps, y0, mode, slope=0.1)[0], ref, bound) > 1e3
            assert rr.ratio(rr.adain_ref(x, w, eps, y0, (mode + 1) % 3)[0], ref, bound) > 1e3


def test_run_probe_and_row_noise():
    a = np.random.Generator(np.random.PCG64(1)).standard_normal(5000).astype(np.float32)
    b = np.random.Generator(np.random.PCG64(2)).standard_normal(5000).astype(np.float32)
    assert not rr.shares_run(a, b) and rr.shares_run(a, np.concatenate([b[:100], a[40:48], b[100:]]))
    # row_noise: the slices of a batch's blocks, laid out as a B = 1 call's (sizes and contents)
    from oracle.synth import refinegan_noise_sizes

    cfg = rr.config("rg_32k")
    B, T, Tb = 3, 4, 3
    sizes = refinegan_noise_sizes(cfg, B, T)
    flat = np.arange(sum(sizes), dtype=np.float32)
    one = rr.row_noise(cfg, flat, B, T, 1, Tb)
    s1 = refinegan_noise_sizes(cfg, 1, Tb)
    assert one.size == sum(s1)
    p = np.split(one, np.cumsum(s1)[:-1])
    assert p[0][0] == T * cfg.upp and p[1][0] == sizes[0] + 1  # row 1's first source sample, its phase
    blk = flat[sizes[0] + sizes[1]:sizes[0] + sizes[1] + sizes[2]].reshape(B, 256, T * 10)
    assert np.array_equal(p[2].reshape(256, Tb * 10), blk[1, :, :Tb * 10])


# ----------------------------------------------------------------- 2. the module bar
class _Proxy:
    """A module whose named attributes are replaced and every other one passed through."""

    def __init__(self, mod, **over):
        self._mod, self._over = mod, over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(self._mod, k)


def _slope_01(F, nu):
    """F.leaky_relu with the AdaIN / ResBlock calls of refinegan_generator at slope 0.1: the calls come in a fixed
    order -- nu in the down branch, then per stage one before the upsample and 3 x (AdaIN, 6 ResBlock, AdaIN)."""
    n = [0]

    def leaky_relu(x, slope=0.01):
        if slope != 0.2:  # the TextEncoder's (0.1): not the decoder's
            return F.leaky_relu(x, slope)
        i = n[0]
        n[0] += 1
        in_block = nu <= i < nu + 25 * nu and (i - nu) % 25 != 0
        return F.leaky_relu(x, 0.1 if in_block else slope)

    return leaky_relu


def _align_corners(F):
    def interpolate(x, size=None, scale_factor=None, mode="nearest"):
        if mode == "linear" and scale_factor is not None:  # the stages' nn.Upsample (the f0 one passes size=)
            return F.interpolate(x, size=int(x.shape[-1] * scale_factor), mode="linear", align_corners=True)
        return F.interpolate(x, size=size, scale_factor=scale_factor, mode=mode)

    return interpolate


def _width_off_by_one(real):
    import math

    import torch.nn.functional as F

    from oracle.realtime import sinc_resample_kernel

    def functional_resample(w, orig_freq, new_freq, **kw):
        kernel, width, orig, new = sinc_resample_kernel(orig_freq, new_freq, kw["lowpass_filter_width"], kw["rolloff"],
                                                        w.dtype, kw["resampling_method"], kw["beta"])
        shape = w.size()
        v = F.pad(w.reshape(-1, shape[-1]), (width - 1, width + orig + 1))  # the taps read one row late
        y = F.conv1d(v[:, None], kernel, stride=orig).transpose(1, 2).reshape(v.shape[0], -1)
        target = int(math.ceil(new * shape[-1] / orig))
        return y[..., :target].reshape(shape[:-1] + (target,))

    return functional_resample


def _mean_over_two(torch_mod):
    def stack(tensors, dim=0):
        s = torch_mod.stack(tensors, dim=dim)
        return s * 1.5 if len(tensors) == 3 else s  # sum / 2 where the reference takes sum / 3

    return stack


def _ada_parts(cfg, B, T):
    from oracle.synth import refinegan_noise_sizes

    return np.cumsum([0] + refinegan_noise_sizes(cfg, B, T))


def test_module_bar_sees_decoder_mistakes(monkeypatch):
    import oracle.realtime as orealtime
    import oracle.synth as osynth

    cfg, w = rr.config("rg_48k"), rr.weights_for("rg_48k")
    c = rr.synth_case(cfg)
    B, T = len(rr.LENGTHS), rr.LENGTHS[0]
    ref, gap = anchor(pa.synth_fn(w, cfg=cfg, **c))["o"]
    peak = float(np.abs(ref).max())
    bar = K * max(gap, pa.ULP32 * peak)

    def run(eps_src=None):
        cc = dict(c, eps_src=c["eps_src"] if eps_src is None else eps_src)
        return pa._as_dict(pa.synth_fn(w, cfg=cfg, **cc)(torch.float64))["o"]

    assert float(np.abs(run() - ref).max()) == 0.0  # the harness itself changes nothing
    at = _ada_parts(cfg, B, T)
    swapped = c["eps_src"].copy()
    swapped[at[2]:at[3]], swapped[at[3]:at[4]] = c["eps_src"][at[3]:at[4]], c["eps_src"][at[2]:at[3]]
    transposed = c["eps_src"].copy()
    ch, t = 512, T
    k = 2
    for r in cfg.upsample_rates:
        ch, t = ch // 2, t * r
        for _ in range(6):
            transposed[at[k]:at[k + 1]] = c["eps_src"][at[k]:at[k + 1]].reshape(B, t, ch).transpose(0, 2, 1).reshape(-1)
            k += 1
    F = torch.nn.functional
    rows = []

    def deviation(name, patch=None, eps_src=None):
        with monkeypatch.context() as m:
            if patch:
                patch(m)
            err = float(np.abs(run(eps_src) - ref).max())
        rows.append((name, err / peak, err / bar))

    nu = len(cfg.upsample_rates)
    deviation("AdaIN / ResBlock slope 0.1", lambda m: m.setattr(osynth, "F", _Proxy(F, leaky_relu=_slope_01(F, nu))))
    deviation("AdaIN draws of one branch swapped", eps_src=swapped)
    deviation("align_corners=True upsample", lambda m: m.setattr(osynth, "F", _Proxy(F, interpolate=_align_corners(F))))
    deviation("resampler width off by one",
              lambda m: m.setattr(orealtime, "functional_resample", _width_off_by_one(orealtime.functional_resample)))
    deviation("mean of three branches over two",
              lambda m: m.setattr(osynth, "torch", _Proxy(torch, stack=_mean_over_two(torch))))
    deviation("noise read as [B][T][C]", eps_src=transposed)
    print(f"\nrg_48k synth {rr.LENGTHS} waveform: gap {gap / peak:.2e} of the peak, bar K x gap {bar / peak:.2e}")
    for name, e, q in rows:
        print(f"  {name:38s} err {e:.2e} of the peak = {q:9.1f} x the bar{'' if q > 1 else '   UNRESOLVED'}")
    assert float(np.abs(run() - ref).max()) == 0.0  # every patch is gone
    assert all(q > 1 for _, _, q in rows), [n for n, _, q in rows if q <= 1]
