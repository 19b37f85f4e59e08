"""The generators' harmonic sources alone (rvcx_dec_source, include/rvcx_test.h): NSF SineGen (k_sine_cum / k_sine,
csrc/nsf_source.hip) and the 9-harmonic MRF source (csrc/source_harm.hip), whose phase scans claim to be bit-identical
to torch's sequential double-accumulated loops. The noise and, for MRF, the initial phases are injected.

Two checks per case:
  * against oracle.synth.sine_source / harmonic_source in float32 on the CPU, the reference's own arithmetic:
    max |dev - ref32| <= 16 * 2^-24. With a bit-identical scan the argument of sin has the same bits on both sides, and
    what remains is libm against the device's sinf / tanhf (and a contracted multiply-add), a few ulp of an output
    <= 1. A scan that is off by one rem, one frame or one chunk moves the phase by a visible fraction of a cycle.
  * against the oracle in float64 under parity_anchor.check, K = 8, absolute: the loose one (the oracle's own fp32 gap
    reaches 9e-5 on the alternating track at L = 2050, the fp32 rem errors adding up over the frames); it is there
    for the voiced / unvoiced and amplitude handling.

f0 tracks: constant 50, 150 (both on the fmod(inc + 0.5, 1) discontinuity: f0 upp / sr = 0.5, 1.5) and 1100 Hz, all
unvoiced, alternating 220 / 0 per frame, random 50 - 1100 Hz with 30 % of the frames unvoiced.
Lengths: NSF L = 1, 2, 3 and 1025 / 1026 (k_sine_cum's per-thread segment goes from 1 to 2 rems at L - 1 = 1025) and
2050, B = 1 and B = 3; MRF L = 1, 2, 3, 9 (4320 samples: 4 chunks of 1024 and a partial one) and 30, B = 2.
"""
import dataclasses

import numpy as np
import pytest
import torch

from parity_anchor import K, anchor, check

pytestmark = pytest.mark.gpu

SHARP = 16 * 2.0 ** -24
TRACKS = ("const50", "const150", "const1100", "unvoiced", "alt", "random")


def track(name, L, seed=0):
    if name.startswith("const"):
        return np.full(L, float(name[5:]), np.float32)
    if name == "unvoiced":
        return np.zeros(L, np.float32)
    if name == "alt":
        return np.where(np.arange(L) % 2 == 0, 220.0, 0.0).astype(np.float32)
    rng = np.random.default_rng(100 + seed)
    return (rng.uniform(50.0, 1100.0, L) * (rng.uniform(size=L) > 0.3)).astype(np.float32)


@pytest.fixture(scope="module")
def sources(engine, synth_w):
    """get(name) -> (Engine, weights, cfg) for "nsf48" (the session's 48 kHz v2 engine), "nsf40" (tests/synth_configs
    v2_40k) and "mrf" (the MRF HiFi-GAN configuration of tests/test_gpu_vocoders.py); the last two carry a synthesizer
    alone and are made at their first use."""
    import synth_configs
    from rvcx import synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state

    made = {"nsf48": (engine, synth_w, SYNTH_48K_V2)}
    own = []

    def get(name):
        if name not in made:
            if name == "nsf40":
                cfg, w = synth_configs.CONFIGS["v2_40k"], synth_configs.weights_for("v2_40k")
            else:
                cfg = dataclasses.replace(SYNTH_48K_V2, vocoder="MRF HiFi-GAN")
                w = normalize_state(synthetic.synth_state(11, cfg))
            e = Engine(0)
            own.append(e)
            e.load_synth(w, cfg)
            made[name] = (e, w, cfg)
        return made[name]

    yield get
    for e in own:
        e.close()


def lin(w, dt):
    return (torch.as_tensor(np.asarray(w["dec.m_source.l_linear.weight"])).to(dt),
            torch.as_tensor(np.asarray(w["dec.m_source.l_linear.bias"])).to(dt))


def both_checks(name, dev, fn):
    anc = anchor(fn)["out"]
    ref32 = fn(torch.float32).detach().to(torch.float64).numpy()
    assert dev.shape == ref32.shape and np.isfinite(dev).all(), name
    d32 = float(np.abs(dev.astype(np.float64) - ref32).max())
    print(f"\nsource {name}: vs fp32 oracle {d32:.3e} bound {SHARP:.3e} ratio {d32 / SHARP:.3f}")
    check(f"source {name} vs fp64", dev, *anc, K, absolute=True)
    assert d32 <= SHARP, f"source {name}: {d32:.3e} from the fp32 oracle > 16 * 2^-24: the phase scans differ"


def run_nsf(get, which, f0, seed):
    from oracle import synth as osynth

    eng, w, cfg = get(which)
    B, L = f0.shape
    eps = np.random.default_rng(seed).standard_normal((B, L * cfg.upp)).astype(np.float32)
    dev = eng.dec_source(f0, eps_src=eps).cpu().numpy()
    eng.check_device_status()
    tf0, teps = torch.from_numpy(f0), torch.from_numpy(eps)

    def fn(dt):
        return osynth.sine_source(tf0.to(dt), cfg.upp, cfg.sr, teps.to(dt), *lin(w, dt)).reshape(B, -1)

    return dev, fn


NSF_L = [1, 2, 3, 1025, 1026, 2050]


@pytest.mark.parametrize("name", TRACKS)
@pytest.mark.parametrize("L", NSF_L)
def test_nsf_source_tracks(sources, L, name):
    f0 = track(name, L)[None]
    dev, fn = run_nsf(sources, "nsf48", f0, seed=L)
    both_checks(f"nsf48 L={L} {name}", dev, fn)


@pytest.mark.parametrize("rows", [("const150", "alt", "random"), ("const50", "unvoiced", "const1100")])
@pytest.mark.parametrize("L", NSF_L)
def test_nsf_source_batch(sources, L, rows):
    """B = 3 with different rows: one k_sine_cum block per row."""
    f0 = np.stack([track(n, L, seed=i) for i, n in enumerate(rows)])
    dev, fn = run_nsf(sources, "nsf48", f0, seed=50 + L)
    both_checks(f"nsf48 L={L} B=3 {'/'.join(rows)}", dev, fn)


@pytest.mark.parametrize("name", TRACKS)
def test_nsf_source_40k(sources, name):
    """upp = 400, sr = 40000 (tests/synth_configs.py v2_40k) at L = 1026."""
    f0 = track(name, 1026)[None]
    dev, fn = run_nsf(sources, "nsf40", f0, seed=7)
    assert dev.shape == (1, 1026 * 400)
    both_checks(f"nsf40 L=1026 {name}", dev, fn)


@pytest.mark.parametrize("rows", [("const50", "const150"), ("const1100", "unvoiced"), ("alt", "random")])
@pytest.mark.parametrize("L", [1, 2, 3, 9, 30])
def test_mrf_source(sources, L, rows):
    from oracle import synth as osynth

    eng, w, cfg = sources("mrf")
    B, N = 2, L * cfg.upp
    f0 = np.stack([track(n, L, seed=i) for i, n in enumerate(rows)])
    rng = np.random.default_rng(200 + L)
    eps = rng.standard_normal((B, N, 9)).astype(np.float32)
    ini = rng.random((B, 9)).astype(np.float32)
    dev = eng.dec_source(f0, eps_src=np.concatenate([eps.reshape(-1), ini.reshape(-1)])).cpu().numpy()
    eng.check_device_status()
    f0_up = torch.from_numpy(np.repeat(f0, cfg.upp, axis=1)[:, :, None])  # F.interpolate(mode="nearest")
    teps, tini = torch.from_numpy(eps), torch.from_numpy(ini)

    def fn(dt):
        return osynth.harmonic_source(f0_up, cfg.sr, 9, teps, tini, *lin(w, dt)).reshape(B, N)

    assert dev.shape == (B, N)
    both_checks(f"mrf L={L} {'/'.join(rows)}", dev, fn)


def test_dec_source_needs_a_pitch_guided_synth():
    from rvcx import _lib
    from rvcx.engine import Engine

    e = Engine(0)
    try:
        t = e.torch
        f0 = t.zeros((1, 2), dtype=t.float32, device=e.device)
        out = t.zeros((1, 2 * 480), dtype=t.float32, device=e.device)
        rc = e.lib.rvcx_dec_source(e.ctx, 1, 2, f0.data_ptr(), None, 0, out.data_ptr(), e.stream())
        assert _lib.STATUS[rc] == "RVCX_E_STATE"
    finally:
        e.close()
