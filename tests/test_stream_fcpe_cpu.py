"""Realtime streams with f0_method "fcpe", the parts that need no GPU: the conditions under which the reference
fixture (tests/golden/stream_fcpe_4.npz, made by tests/golden/make_golden_stream_fcpe.py) is a meaningful yardstick,
the f0_method validation of rvcx.realtime.VoiceChanger, and a CPU restatement of the "fcpe" stream
(tests/stream_fcpe_ref.py) that reproduces the fixture without sharing code with the script's torchfcpe adapter."""
import hashlib

import numpy as np
import pytest
import torch

import parity_anchor as pa
from conftest import golden
from stream_fcpe_ref import stream_inputs


def test_fixture_conditions():
    """The regenerated inputs hash to the stored digest; every float64 frame maximum lies at least 2 K gaps from the
    stored threshold (the device is within K gaps and the reference's fp32 run within one: no voicing decision can
    flip); at most 25 % of the ungated hops hold an unsure frame; the threshold splits the frames (voiced share in
    [0.2, 0.8]); the gated hops are the ones with vol 0, in the silent stream."""
    g = golden("stream_fcpe_4.npz")
    S, H = int(g["n_streams"]), int(g["hops"])
    x = stream_inputs(g)
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(g["input_sha256"]), "regenerated inputs differ"
    thr, gap = float(g["threshold"]), float(g["gap"])
    mx = g["frame_max64"]
    assert mx.shape == (S, H, 88) and g["out16"].shape == (S, H, int(g["block"])) and g["unsure"].shape == (S, H)
    assert 0 < gap < 1e-3 and float(np.abs(mx - thr).min()) >= 2 * pa.K * gap
    ungated = g["vol"] > 0
    assert int((g["unsure"] & ungated).sum()) <= 0.25 * int(ungated.sum())
    assert 0.2 <= float((mx > thr).mean()) <= 0.8
    gated = np.argwhere(~ungated)
    assert len(gated) >= 1 and all(int(s) == int(g["silent_stream"]) and int(h) in g["silent_hops"] for s, h in gated)
    assert (g["vol"][~ungated] == 0).all() and (g["sola_offset"][~ungated] == 0).all()


def test_voice_changer_validates_f0_method_before_the_engine():
    """The reference's VoiceChanger takes f0_method "rmvpe" or "fcpe"; any other name is refused by name, before the
    engine is looked at (so without a GPU). The supported names pass that check and reach the engine check."""
    from rvcx.realtime import F0_METHODS, VoiceChanger

    assert F0_METHODS == ("rmvpe", "fcpe")
    with pytest.raises(ValueError, match="rmvpe.*fcpe") as e:
        VoiceChanger(96, 0.1, 0.5, engine=None, f0_method="dio")
    assert "dio" in str(e.value)
    for name in F0_METHODS:
        with pytest.raises(ValueError, match="Engine"):
            VoiceChanger(96, 0.1, 0.5, engine=None, f0_method=name)


def test_cpu_restatement_reproduces_the_fixture(synth_w, hubert_w):
    """Stream 0, hops 0-1, through OracleVoiceChanger with the fcpe_ref track at the stored threshold, at the bars of
    tests/test_gpu_stream_ref.py: vol rel <= 1e-5, spectrogram correlation >= 0.999, max |diff| <= 2e-3 of the peak
    where the SOLA offset agrees, and the offsets agree (hops flagged unsure are exempt from the last three)."""
    from oracle.metrics import spectrogram_correlation
    from rvcx import synthetic
    from rvcx.config import HUBERT_BASE, SYNTH_48K_V2
    from rvcx.weights import check_fcpe_state, fcpe_sizes
    from stream_fcpe_ref import FcpeOracleVoiceChanger

    g = golden("stream_fcpe_4.npz")
    blk, s = int(g["block"]), 0
    x = stream_inputs(g)
    cfg = synthetic.fcpe_config(int(g["fcpe_layers"]), int(g["fcpe_chans"]))
    fw = pa.cast_weights(check_fcpe_state(synthetic.fcpe_state(int(g["fcpe_seed"]), int(g["fcpe_layers"]),
                                                              int(g["fcpe_chans"])), cfg), torch.float32)
    rng = np.random.Generator(np.random.PCG64(int(g["noise_seed0"]) + s))
    vc = FcpeOracleVoiceChanger(synth_w, SYNTH_48K_V2, hubert_w, HUBERT_BASE, fw, fcpe_sizes(cfg),
                                fcpe_threshold=float(g["threshold"]), read_chunk_size=96, silent_threshold=-90,
                                sid=int(g["sids"][s]),
                                noise_fn=lambda shape, which: torch.from_numpy(
                                    rng.standard_normal((1, *shape[1:]) if which == "z" else (1, shape[1], 1))
                                    .astype(np.float32).reshape(shape)))
    for h in range(2):
        out, vol = vc.on_request(x[s, h * blk:(h + 1) * blk].copy(), f0_up_key=int(g["f0_up_key"]), index_rate=0.0,
                                 protect=float(g["protect"]))
        ref, rv = g["out16"][s, h].astype(np.float32), float(g["vol"][s, h])
        assert rv > 0 and abs(vol - rv) <= 1e-5 * rv
        assert np.isfinite(out).all()
        if bool(g["unsure"][s, h]):
            continue
        assert vc.last["sola_offset"] == int(g["sola_offset"][s, h]), (h, vc.last["sola_offset"])
        assert spectrogram_correlation(out, ref) >= 0.999, h
        assert float(np.abs(out - ref).max()) <= 2e-3 * float(np.abs(ref).max()), h
