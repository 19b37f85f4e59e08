"""Module outputs of the HIP path against the oracle in float64, each held to K = 8 times the oracle's own
fp32-vs-fp64 gap on the same inputs (tests/parity_anchor.py): HuBERT features (v2, v1, batched), the RMVPE salience
from audio (with the reflect-padded frame counts, batched) and the decode decisions it implies, every output of
Synthesizer.infer (m_p, logs_p, z_p, z, waveform; T = 1, ragged batch, speaker rows beyond 0, coarse pitch 1 and 255,
unvoiced rows, rate) and the generator alone on the oracle's z. What the whole-module outputs see only through these:
LayerNorm, GroupNorm, GELU, the WaveNet gate, the sine source, conv_post, the STFT magnitude and mel projection,
avg-pool, BatchNorm folding, the BiGRU, the gathers and masks, and the runtime glue between them.

Every point prints `name: err bound err/gap`. tests/test_parity_anchor_cpu.py shows which deviations these bars catch.
"""
import numpy as np
import pytest
import torch

import parity_anchor as pa
from parity_anchor import K, anchor, check, check_each
from rmvpe_parity import check_salience

pytestmark = pytest.mark.gpu


def speech(n, seed):
    from rvcx import synthetic

    return synthetic.speech_like(n, seed=seed).astype(np.float32)


# ----------------------------------------------------------------- HuBERT
@pytest.mark.parametrize("n,version", [(400, "v2"), (5000, "v2"), (10080, "v2"), (10080, "v1"), (16000, "v2")])
def test_hubert_vs_fp64(engine, hubert_w, n, version):
    """L = 1, 15, 31, 49 frames; v1 adds final_proj (768 -> 256)."""
    audio = speech(n, seed=40)
    ref, gap = anchor(pa.hubert_fn(hubert_w, audio[None], version))["out"]
    f = engine.host(engine.hubert(audio, version=version))
    assert ref.shape == (1, {400: 1, 5000: 15, 10080: 31, 16000: 49}[n], 256 if version == "v1" else 768)
    check(f"hubert {version} n={n}", f, ref[0], gap, K)


def test_hubert_batch_vs_fp64(engine, hubert_w):
    B, n = 3, 5000
    audio = np.stack([speech(n, seed=41 + b) for b in range(B)])
    f = engine.host(engine.hubert_batch(audio))
    assert f.shape == (B, 15, 768)
    for b in range(B):  # each row against its own float64 output and its own gap
        ref, gap = anchor(pa.hubert_fn(hubert_w, audio[b:b + 1]))["out"]
        check(f"hubert_batch row {b} n={n}", f[b], ref[0], gap, K)


# ----------------------------------------------------------------- RMVPE
@pytest.mark.parametrize("n", [2720, 4960, 5280, 16000])
def test_rmvpe_salience_vs_fp64(engine, rmvpe_w, n):
    """F = 18 (reflect pad 14), 32 (none), 34 (pad 30 of at most 33), 101 frames; the reference is float64 from the
    audio on: STFT, mel projection, log, U-Net, BiGRU."""
    audio = speech(n, seed=50)
    ref, gap = anchor(pa.rmvpe_fn(rmvpe_w, audio[None]))["out"]
    f0, hid = engine.rmvpe(audio, 0.03, want_hidden=True)
    f0, hid = engine.host(f0), engine.host(hid)
    assert hid.shape == ref[0].shape == (1 + n // 160, 360)
    check_salience(f"rmvpe n={n}", f0, hid, ref[0], gap)


def test_rmvpe_batch_salience_vs_fp64(engine, rmvpe_w):
    B, n = 2, 5280
    audio = np.stack([speech(n, seed=51 + b) for b in range(B)])
    f0, hid = engine.rmvpe_batch(audio, 0.03, want_hidden=True)
    f0, hid = engine.host(f0), engine.host(hid)
    assert hid.shape == (B, 34, 360)
    for b in range(B):
        ref, gap = anchor(pa.rmvpe_fn(rmvpe_w, audio[b:b + 1]))["out"]
        check_salience(f"rmvpe_batch row {b} n={n}", f0[b], hid[b], ref[0], gap)


# ----------------------------------------------------------------- synthesizer
def run_synth(engine, c, rate=None):
    out = engine.synth_infer_ex(c["phone"], c["lengths"], c["pitch"], c["f0"], c["sid"], rate=rate, eps_z=c["eps_z"],
                                eps_src=c["eps_src"])
    return dict(zip(("o", "z_p", "z", "m_p", "logs_p"), (engine.host(v) for v in out)))


@pytest.mark.parametrize("lengths", [(1,), (24,), (40, 29, 1)])
def test_synth_vs_fp64(engine, synth_w, lengths):
    """All five outputs, each relative to its own peak, in the order of the chain (m_p / logs_p -> z_p -> z ->
    waveform): the first one over the bar is where the deviation enters."""
    c = pa.synth_case(lengths, seed=60)
    coarse = set(c["pitch"].reshape(-1).tolist())
    assert tuple(c["sid"]) == pa.SIDS[:len(lengths)] and 255 in coarse and (1 in coarse or c["pitch"].size == 1)
    assert len(lengths) == 1 or not c["f0"][-1].any()
    anc = anchor(pa.synth_fn(synth_w, **c))
    dev = run_synth(engine, c)
    check_each([(f"synth {lengths} {k}", dev[k], *anc[k], K) for k in ("m_p", "logs_p", "z_p", "z", "o")])


def test_synth_rate_vs_fp64(engine, synth_w):
    """rate 0.5 at T = 24: z_p, z and the waveform cover the last 12 frames."""
    c = pa.synth_case((24,), seed=61, rate=0.5)
    anc = anchor(pa.synth_fn(synth_w, rate=0.5, **c))
    dev = run_synth(engine, c, rate=0.5)
    assert dev["z"].shape == (1, 12, 192) and dev["o"].shape == (1, 12 * engine.upp)
    check_each([(f"synth rate 0.5 {k}", dev[k], *anc[k], K) for k in ("z_p", "z", "o")])


def test_dec_only_vs_fp64(engine, synth_w):
    """The generator alone at (B, T) = (2, 24): the oracle's float64 z rounded to fp32 goes to both oracle dtypes and
    to the device, so the waveform error here is the generator's own."""
    c = pa.synth_case((24, 24), seed=62)
    z = pa.synth_fn(synth_w, **c)(torch.float64)["z"].transpose(1, 2).numpy().astype(np.float32)
    ref, gap = anchor(pa.dec_fn(synth_w, z, c["f0"], c["sid"], c["eps_src"]))["out"]
    o = engine.host(engine.dec_only(z, c["f0"], c["sid"], eps_src=c["eps_src"]))
    check("dec_only (2, 24)", o, ref, gap, K)
