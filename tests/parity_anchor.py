"""Module parity anchored on the oracle in float64 (test helper, no GPU needed).

The oracle (oracle/*.py) follows the dtype of its weights and inputs. Run in float64 it is the exact answer for
practical purposes; run in float32 it shows how far honest fp32 arithmetic of the same network lands from that answer
on the very inputs of the test: the `gap`. A device output is then held to a small multiple K of the gap instead of to
a bar chosen once.

K is derived, not tuned: the default two-plane contraction arithmetic is allowed 4x the native-fp32 error at kernel
level (test_gpu_conv_math.py), and a device with other kernels and summation orders is granted a factor 2 over the
reference's own gap (tests/rmvpe_parity.py). K = 8 against float64; against a stored fp32 fixture, which itself sits
one gap from float64, the bound is (K + 1) gap.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

K = 8
ULP32 = 2.0 ** -23  # one fp32 ulp of the largest element, relative to it


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))


def cast_weights(w, dtype):
    """State dict -> torch tensors, the floating ones in `dtype` (integer entries such as num_batches_tracked stay)."""
    out = {}
    for k, v in w.items():
        t = _t(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


_CAST = {}


def weights(w, dtype):
    """cast_weights, kept per (state dict, dtype): the session fixtures are cast once for all tests."""
    key = (id(w), dtype)
    if key not in _CAST:
        _CAST[key] = (w, cast_weights(w, dtype))
    return _CAST[key][1]


def _as_dict(v):
    v = v if isinstance(v, dict) else {"out": v}
    return {k: _t(x).detach().to(torch.float64).numpy() for k, x in v.items()}


def anchor(fn):
    """fn(dtype) -> tensor or {name: tensor}. Runs fn(float64) once and fn(float32) on 1 and on 8 threads (one run's
    maximum moves by up to ~30 % with the summation order the thread count selects) and returns
    {name: (ref64, gap)}: the float64 output and the larger of the two max |fp32 - fp64| (absolute)."""
    n0 = torch.get_num_threads()
    try:
        ref = _as_dict(fn(torch.float64))
        gap = {k: 0.0 for k in ref}
        for nt in (1, 8):
            torch.set_num_threads(nt)
            got = _as_dict(fn(torch.float32))
            for k in ref:
                assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
                gap[k] = max(gap[k], float(np.abs(got[k] - ref[k]).max()))
    finally:
        torch.set_num_threads(n0)
    return {k: (ref[k], gap[k]) for k in ref}


def check(name, dev, ref64, gap, K, absolute=False):
    """err = max |dev - ref64| must stay <= K max(gap, 2^-23). err and gap (absolute, as anchor returns it) are both
    taken relative to max |ref64| unless `absolute` (the salience lives in [0, 1]: rmvpe_parity.py). Prints
    `name err bound err/gap` and returns err."""
    dev = np.asarray(_t(dev).detach().cpu().numpy() if isinstance(dev, torch.Tensor) else dev, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert dev.shape == ref64.shape, (name, dev.shape, ref64.shape)
    assert np.isfinite(dev).all(), f"{name}: non-finite output"
    scale = 1.0 if absolute else float(np.abs(ref64).max())
    if scale == 0.0:
        scale = 1.0
    err = float(np.abs(dev - ref64).max()) / scale
    gap = float(gap) / scale
    bound = K * max(gap, ULP32)
    print(f"\n{name}: err {err:.3e} bound {bound:.3e} err/gap {err / gap if gap > 0 else float('inf'):.2f}")
    assert err <= bound, f"{name}: err {err:.3e} > {K} x gap {gap:.3e} = {bound:.3e}"
    return err


def check_each(points):
    """check(*p) for every point, so that each prints its line, then one assertion for all that failed: along a chain
    (m_p / logs_p -> z_p -> z -> waveform) the first one named is where the deviation enters."""
    failed = []
    for p in points:
        try:
            check(*p)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


# ----------------------------------------------------------------- seeded inputs
SIDS = (3, 0, 108)  # the speaker gather beyond row 0, up to the table's last row (spk_embed_dim 109)


def synth_case(lengths, seed, rate=None, upp=480, inter=192, cfg=None):
    """Synthesizer.infer inputs for B = len(lengths) rows of T = lengths[0] frames (PCG64): coarse pitch holding both
    1 and 255 (when there are two frames to hold them), f0 with a voiced/unvoiced/voiced run in row 0 and the last
    row of a batch fully unvoiced, eps_src over the frames the decoder runs on. With `cfg` (a SynthConfig) the phone
    width, upp and the latent width are the configuration's."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, T = len(lengths), int(lengths[0])
    width = 768
    if cfg is not None:
        width, upp, inter = cfg.text_enc_hidden_dim, cfg.upp, cfg.inter_channels
    phone = rng.standard_normal((B, T, width)).astype(np.float32)
    pitch = rng.integers(1, 256, size=(B, T)).astype(np.int64)
    pitch.reshape(-1)[-1] = 255
    if pitch.size > 1:
        pitch.reshape(-1)[0] = 1
    f0 = (110.0 + 250.0 * rng.random((B, T))).astype(np.float32)
    f0[0, T // 3:(2 * T) // 3] = 0.0
    if B > 1:
        f0[-1] = 0.0
    head = 0 if rate is None else int(T * (1.0 - float(rate)))
    eps_z = rng.standard_normal((B, inter, T)).astype(np.float32)
    eps_src = rng.standard_normal((B, (T - head) * upp)).astype(np.float32)
    return dict(phone=phone, lengths=np.asarray(lengths, np.int64), pitch=pitch, f0=f0,
                sid=np.asarray(SIDS[:B], np.int64), eps_z=eps_z, eps_src=eps_src)


# ----------------------------------------------------------------- the oracle as fn(dtype)
def hubert_fn(w, audio, version="v2"):
    """audio [B, n] float32 -> fn(dtype) = HuBERT features [B, L, D]."""
    from oracle import hubert as ohub
    from rvcx.config import HUBERT_BASE

    a = _t(np.asarray(audio, np.float32))
    return lambda dt: ohub.hubert_forward(weights(w, dt), HUBERT_BASE, a.to(dt), version)


def rmvpe_fn(w, audio):
    """audio [B, n] float32 -> fn(dtype) = salience [B, F, 360] from the audio: mel and E2E both in dtype."""
    from oracle import rmvpe as orm
    from rvcx.config import RMVPE_CFG

    a = _t(np.asarray(audio, np.float32))
    return lambda dt: orm.mel2hidden(weights(w, dt), RMVPE_CFG, orm.mel_spectrogram(a.to(dt)))


def synth_fn(w, phone, lengths, pitch, f0, sid, eps_z, eps_src, rate=None, cfg=None):
    """fn(dtype) = Synthesizer.infer's {o [B, T' upp], z_p, z [B, T', I], m_p, logs_p [B, T, I]} in the device's
    time-major layout, for the configuration `cfg` (default SYNTH_48K_V2)."""
    from oracle import synth as osynth
    from rvcx.config import SYNTH_48K_V2

    cfg = SYNTH_48K_V2 if cfg is None else cfg

    f = lambda x: _t(np.asarray(x, np.float32))  # noqa: E731
    i = lambda x: _t(np.asarray(x, np.int64))  # noqa: E731
    phone, f0, eps_z, eps_src = f(phone), f(f0), f(eps_z), f(eps_src)
    lengths, pitch, sid = i(lengths), i(pitch), i(sid)

    def fn(dt):
        o, _, (z, z_p, m_p, logs_p) = osynth.synth_infer(weights(w, dt), cfg, phone.to(dt), lengths, pitch,
                                                         f0.to(dt), sid, eps_z.to(dt), eps_src.to(dt), rate)
        tm = lambda x: x.transpose(1, 2)  # noqa: E731
        return {"o": o.reshape(o.shape[0], -1), "z_p": tm(z_p), "z": tm(z), "m_p": tm(m_p), "logs_p": tm(logs_p)}

    return fn


def dec_fn(w, z, f0, sid, eps_src, cfg=None):
    """z [B, I, T] float32 -> fn(dtype) = the generator's waveform [B, T upp], for `cfg` (default SYNTH_48K_V2)."""
    from oracle import synth as osynth
    from rvcx.config import SYNTH_48K_V2

    cfg = SYNTH_48K_V2 if cfg is None else cfg

    z, f0, eps_src = (_t(np.asarray(x, np.float32)) for x in (z, f0, eps_src))
    sid = _t(np.asarray(sid, np.int64))

    def fn(dt):
        o = osynth.dec_only(weights(w, dt), cfg, z.to(dt), f0.to(dt), sid, eps_src.to(dt))
        return o.reshape(o.shape[0], -1)

    return fn


class PatchedF:
    """torch.nn.functional with some functions replaced, to stand in for an oracle module's `F`."""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(F, k)


def ratios(fn, anc, absolute=False):
    """The fp32 oracle's distance to float64 per output, in units of max(gap, floor): what check() compares to K."""
    got = _as_dict(fn(torch.float32))
    out = {}
    for k, (ref, gap) in anc.items():
        floor = ULP32 * (1.0 if absolute else float(np.abs(ref).max()))
        out[k] = float(np.abs(got[k] - ref).max()) / max(gap, floor)
    return out


def anchored(name, dev, stored, ref64, gap, old_bar, absolute=False):
    """The stored reference output within 2 gap of float64, then the device within (K + 1) gap of the stored output;
    the measured error is printed beside the fixed bar it also passed."""
    stored = np.asarray(stored).reshape(ref64.shape)
    check(f"{name} fixture vs fp64", stored, ref64, gap, 2, absolute)
    err = check(f"{name} device vs fixture", np.asarray(dev).reshape(ref64.shape), stored, gap, K + 1, absolute)
    print(f"{name}: measured {err:.3e}, fixed bar {old_bar:g}")
