"""The FCPE pitch network on device (f0 method "fcpe" of rvc/, rvc/lib/predictors/FCPE.py): the Performer attention
kernels against float64 at kernel level, the salience from audio against the float64 restatement (tests/fcpe_ref.py)
and the reference's own run (tests/golden/fcpe_l2.npz), the decoders and post_process, and the pipeline wiring.

Bounds follow tests/parity_anchor.py: the device stays within K = 8 times the distance of an honest fp32 evaluation
of the same operations from float64 on the same inputs (the gap), (K + 1) gaps from a stored fp32 run. The conditions
that make these checks meaningful (a moving peak bin, a threshold that splits the frames, exponents far from
overflow, few frames near a decision) are asserted on the reference in tests/test_fcpe_cpu.py."""
import numpy as np
import pytest
import torch

import fcpe_ref as fr
import parity_anchor as pa
from conftest import golden
from fcpe_ref import attention_operands as _attention_operands

pytestmark = pytest.mark.gpu

LENGTHS = (15000, 1000, 400)


@pytest.fixture(scope="module")
def fcpe(engine):
    """The fixture, the seeded 2-layer model loaded into the session engine, and per input length the audio with
    the anchored float64 salience and its fp32 gap (computed once for all tests)."""
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, fcpe_sizes

    g = golden("fcpe_l2.npz")
    cfg = synthetic.fcpe_config(int(g["n_layers"]), int(g["n_chans"]))
    raw = synthetic.fcpe_state(int(g["seed"]), int(g["n_layers"]), int(g["n_chans"]))
    z = fcpe_sizes(cfg)
    w = check_fcpe_state(raw, cfg)
    engine.load_fcpe(raw, cfg)
    cases = {}
    for n in LENGTHS:
        audio = synthetic.speech_like(n, seed=int(g["audio_seed"])).astype(np.float32)
        a = torch.from_numpy(audio)
        ref64, gap = pa.anchor(lambda dt, a=a: fr.salience_from_audio(pa.weights(w, dt), z, a.to(dt)))["out"]
        cases[n] = (audio, ref64, gap)
    return dict(g=g, cfg=cfg, raw=raw, z=z, w=w, cases=cases)


# ---------------------------------------------------------------- Performer attention, kernel level
@pytest.mark.parametrize("pscale", [1.0, 30.0])
@pytest.mark.parametrize("T", [7, 94, 301])
def test_performer_attention_is_fp32_accurate(engine, T, pscale):
    """T = 7 (below one 16-row time tile), 94 (ragged, one reduction slab), 301 (three 128-row slabs, the last
    ragged). 266 features are no multiple of the 16-wide MFMA tile. The kernels clamp the loads of the padded
    feature columns to P's last row, so an unmasked padded column would be a second copy of column 265: it would
    count twice in ksum, ctx and the denominator, an error of order 1 / 266 of the output and far above the bound,
    at either scale of P; it could not move rowmax (a copy never exceeds the maximum), so the index mask on rowmax
    is not what these cases exercise."""
    q, k, v, P = _attention_operands(T, pscale, 1000 * T + int(pscale))
    t = torch.from_numpy
    top = float(fr.dash_minus_diag_k(t(k).double(), t(P).double()).max())
    assert top < 60.0, top  # exp stays far below fp32's overflow (e^88)
    ref64, gap = pa.anchor(lambda dt: fr.performer_attention(t(q).to(dt), t(k).to(dt), t(v).to(dt), t(P).to(dt)))["out"]
    out = engine.performer_attention(q, k, v, P)
    pa.check(f"performer T={T} P x{pscale:g} (max exponent {top:.1f})", out, ref64, gap, pa.K)
    if T == 301:  # slabs are combined in slab order, without atomics: run-to-run bit identical
        assert torch.equal(engine.performer_attention(q, k, v, P), out)


# ---------------------------------------------------------------- salience from audio
@pytest.mark.parametrize("n", LENGTHS)
def test_salience_vs_fp64_and_fixture(engine, fcpe, n):
    """n = 15000 (94 frames), 1000 (7 frames, reflect padding), 400 (3 frames, the zero-padding branch): the device
    salience within K gaps of float64 (absolute: the outputs live in [0, 1]) and (K + 1) gaps of the reference's
    fp32 run."""
    audio, ref64, gap = fcpe["cases"][n]
    f0, sal = engine.fcpe(audio, float(fcpe["g"][f"thr_{n}"]), want_salience=True)
    assert sal.shape == ref64.shape == (n // 160 + 1, 360) and f0.shape == (n // 160 + 1,)
    pa.check_each([(f"fcpe salience n={n} vs fp64", sal, ref64, gap, pa.K, True),
                   (f"fcpe salience n={n} vs fixture", sal, fcpe["g"][f"sal_{n}"], gap, pa.K + 1, True)])


@pytest.mark.parametrize("n", LENGTHS)
def test_mel_vs_fp64_and_fixture(engine, fcpe, n):
    """The network's input on its own (rvcx_fcpe_mel), all 128 bands: the seeded model's first conv weighs the bands
    around 22, so the salience checks say little about the rest of the mel (the logarithmic part of the Slaney
    basis, the upper STFT bins, the magnitude's floor). Held to K gaps of the float64 restatement and (K + 1) gaps of
    the reference's own fp32 mel, the gap being the fp32 restatement's distance from float64 on this audio (at
    n = 15000 it is set by the bands at the fp32 FFT's rounding floor, ~3e-3 in the log-mel), relative to the
    largest |log-mel| (11.5, the clamp)."""
    audio, _, _ = fcpe["cases"][n]
    a = torch.from_numpy(audio)
    ref64, gap = pa.anchor(lambda dt: fr.mel(fcpe["z"], a.to(dt)))["out"]
    mel = engine.fcpe_mel(audio)
    assert mel.shape == ref64.shape == (n // 160 + 1, 128)
    err = np.abs(mel.cpu().numpy() - ref64).max(0)
    print(f"\nfcpe mel n={n}: worst band {int(err.argmax())}, max err by band group (0-31, 32-63, 64-95, 96-127): "
          + " ".join(f"{err[i:i + 32].max():.2e}" for i in range(0, 128, 32)))
    pa.check_each([(f"fcpe mel n={n} vs fp64", mel, ref64, gap, pa.K),
                   (f"fcpe mel n={n} vs fixture", mel, fcpe["g"][f"mel_{n}"], gap, pa.K + 1)])


def test_end_to_end_f0(engine, fcpe):
    """n = 15000: the device f0 is the decode of the device's own salience (rtol 2e-6), and peak bin and voicing equal
    the float64 reference's on every frame whose fp64 top-2 margin and distance to the threshold are at least K gaps;
    the frames excluded are at most 2 % (test_fcpe_cpu.py shows the reference alone stays inside that)."""
    n = 15000
    audio, ref64, gap = fcpe["cases"][n]
    thr = float(fcpe["g"][f"thr_{n}"])
    f0, sal = engine.fcpe(audio, thr, want_salience=True)
    f0, sal = f0.cpu().numpy(), sal.cpu().numpy()
    want = fr.decode(torch.from_numpy(sal), torch.from_numpy(fcpe["w"]["cent_table"]), thr).numpy()
    np.testing.assert_array_equal(f0 > 0, want > 0)
    np.testing.assert_allclose(f0, want, rtol=2e-6, atol=0)
    assert np.array_equal(f0.astype(np.float32).astype(np.float64), f0)  # the raw track holds fp32 values
    srt = np.sort(ref64, axis=1)
    mx64 = ref64.max(1)
    sure = (srt[:, -1] - srt[:, -2] >= pa.K * gap) & (np.abs(mx64 - thr) >= pa.K * gap)
    print(f"\nfcpe e2e: {int((~sure).sum())} of {len(sure)} frames within {pa.K} x gap {gap:.2e} of a decision; "
          f"voiced {float((f0 > 0).mean()):.2f}")
    assert (~sure).mean() <= 0.02
    np.testing.assert_array_equal(sal.argmax(1)[sure], ref64.argmax(1)[sure])
    np.testing.assert_array_equal((f0 > 0)[sure], (mx64 > thr)[sure])
    assert 0.2 <= (f0 > 0).mean() <= 0.8 and len(np.unique(sal.argmax(1))) >= 20


# ---------------------------------------------------------------- decode alone
def _structured_salience(F, seed):
    """Sigmoid-like outputs with a moving pitch track (a vibrato and an octave jump), stretches pinned to the first
    and last bins (the +-4 window clamps at 0 and 359) and an unvoiced gap; no frame maximum lies within 1e-3 of the
    0.5 threshold (peaks 0.8 - 0.95, background and gap below 0.35)."""
    rng = np.random.default_rng(seed)
    t = np.arange(F)
    track = 150 + 40 * np.sin(2 * np.pi * t / 90.0)
    track[F // 2:] += 60
    track[10:16] = [0, 1, 2, 3, 1, 0]
    track[F - 16:F - 10] = [359, 358, 357, 356, 358, 359]
    sal = rng.uniform(0.0, 0.35, size=(F, 360))
    peak = rng.uniform(0.8, 0.95, size=(F, 1))
    sal = np.maximum(sal, peak * np.exp(-0.5 * ((np.arange(360)[None, :] - track[:, None]) / 1.5) ** 2))
    sal[F // 3:F // 3 + 12] = rng.uniform(0.0, 0.3, size=(12, 360))
    return sal.astype(np.float32)


@pytest.mark.parametrize("decoder", ["local_argmax", "argmax"])
def test_decode_vs_reference(engine, fcpe, decoder):
    """rvcx_fcpe_decode on structured salience: f0 at rtol 2e-6 (the CREPE decode test's bar) and voicing exactly,
    for both decoders, windows clamped at bins 0 and 359 included."""
    sal = _structured_salience(400, 9)
    thr = 0.5
    mx = sal.max(1)
    assert np.abs(mx - thr).min() > 1e-3 and 0.02 < (mx <= thr).mean() < 0.1
    assert {0, 1, 359}.issubset(set(sal.argmax(1).tolist()))
    want = fr.decode(torch.from_numpy(sal), torch.from_numpy(fcpe["w"]["cent_table"]), thr, decoder).numpy()
    got = engine.fcpe_decode(sal, thr, decoder).cpu().numpy()
    np.testing.assert_array_equal(got > 0, want > 0)
    np.testing.assert_array_equal(got > 0, mx > thr)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
    if decoder == "local_argmax":
        assert len(np.unique(np.round(want[want > 0]))) > 20


# ---------------------------------------------------------------- post_process (interp_uv, pad_to)
@pytest.mark.parametrize("n", LENGTHS)
def test_interp_uv_and_pad_to(engine, fcpe, n):
    """FCPEF0Predictor.compute_f0's tail for pad_to = F - 1 (its default p_len), F and 2 F: on the reference's own
    salience the device gives the fixture's compute_f0 track (rtol 2e-6: the decode's bar; the interpolation itself
    is fp64), and from audio it equals the restated post_process of the device's own raw track."""
    g = fcpe["g"]
    audio, _, _ = fcpe["cases"][n]
    thr = float(g[f"thr_{n}"])
    F = n // 160 + 1
    raw = engine.fcpe(audio, thr).cpu().numpy()
    for pad_to in (F - 1, F, 2 * F):
        got = engine.fcpe_decode(g[f"sal_{n}"], thr, interp_uv=True, pad_to=pad_to).cpu().numpy()
        want = g[f"interp_{n}_{pad_to}"]
        assert got.shape == want.shape == (pad_to,)
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
        own = engine.fcpe(audio, thr, interp_uv=True, pad_to=pad_to).cpu().numpy()
        np.testing.assert_allclose(own, fr.post_process(raw, 160, 16000, pad_to), rtol=1e-12, atol=0)
    np.testing.assert_allclose(engine.fcpe(audio, thr, interp_uv=True).cpu().numpy(),
                               fr.post_process(raw, 160, 16000), rtol=1e-12, atol=0)
    # no voiced frame (threshold above every maximum): zeros, as compute_f0 returns (:908-909)
    assert not engine.fcpe(audio, 1.0, interp_uv=True, pad_to=F + 3).cpu().numpy().any()


# ---------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def speech():
    from rvcx import synthetic

    return synthetic.speech_like(24000, seed=7)


def test_pipeline_fcpe(engine, fcpe, speech):
    """PipelineRVCX(semantics="rvc", fcpe_weights=(state, config)): get_f0 is rvcx_fcpe + f0_post bit for bit; the
    device pipeline (rvcx_pipeline_opts.f0_method 3) is finite and decodes FCPE on the high-passed, t_pad-padded
    input; without fcpe_weights "fcpe" still raises, and semantics="mlx" keeps the RMVPE fallback whatever is given."""
    from rvcx.infer import Config, HubertModel, PipelineMLX, RMVPE0Predictor, Synthesizer

    weights = (fcpe["raw"], fcpe["cfg"])
    thr = 0.5
    pl = PipelineMLX(48000, Config(), HubertModel(engine), RMVPE0Predictor(engine), semantics="rvc",
                     fcpe_weights=weights, fcpe_threshold=thr)
    x = speech
    coarse, f0 = pl.get_f0(x, len(x) // 160, f0_method="fcpe")
    ref = engine.fcpe(x.astype(np.float32), thr)
    assert 0.1 < float((ref > 0).double().mean()) < 0.9
    c_ref, _, f_ref = engine.f0_post(ref, 0.0)
    np.testing.assert_array_equal(coarse, c_ref.cpu().numpy())
    np.testing.assert_array_equal(f0, f_ref.cpu().numpy())
    y = pl.pipeline(None, Synthesizer(engine), 0, x, f0_method="fcpe", seed=3)
    assert y.ndim == 1 and np.isfinite(y).all() and np.abs(y).max() > 0
    _, p32 = engine.highpass_pad(x, pl.t_pad)
    want = engine.f0_post(engine.fcpe(p32, thr), 0.0)[2]
    np.testing.assert_array_equal(pl.last_f0.cpu().numpy(), want.cpu().numpy())
    with pytest.raises(ValueError, match="fcpe_weights"):
        PipelineMLX(48000, Config(), HubertModel(engine), RMVPE0Predictor(engine), semantics="rvc",
                    f0_method="fcpe")
    with pytest.raises(ValueError, match="fcpe_weights"):
        PipelineMLX(48000, Config(), HubertModel(engine), RMVPE0Predictor(engine)).get_f0(x, 0, f0_method="fcpe")
    mlx = PipelineMLX(48000, Config(), HubertModel(engine), RMVPE0Predictor(engine), semantics="mlx",
                      fcpe_weights=weights)
    _, f0m = mlx.get_f0(x, len(x) // 160, f0_method="fcpe")
    np.testing.assert_array_equal(f0m, engine.f0_post(engine.rmvpe(x.astype(np.float32), 0.03), 0.0)[2].cpu().numpy())


def test_pipeline_batch_and_workspace_fcpe(engine, fcpe, speech):
    """rvcx_pipeline_batch with f0_method 3: each row's adjusted f0 equals rvcx_pipeline_ex's on that utterance alone.
    rvcx_workspace_bytes under f0_method 3 is at least its value under 0, and a call inside a caller-owned arena of
    that size succeeds with the same result."""
    engine.load_fcpe(fcpe["raw"], fcpe["cfg"])
    engine.set_pipeline_highpass()
    x = np.stack([speech, 0.7 * np.roll(speech, 4000)])
    opts = engine.pipeline_opts(f0_method=3, fcpe_threshold=0.5, protect=0.33)
    y, f0 = engine.pipeline_batch(x, opts, sids=0, seed=3, want_f0=True)
    assert torch.isfinite(y).all()
    singles = []
    for b in range(2):
        yb, f0b = engine.pipeline_ex(x[b], opts, seed=3, want_f0=True)
        singles.append(yb.cpu())
        np.testing.assert_array_equal(f0[b].cpu().numpy(), f0b.cpu().numpy())
        assert 0.1 < float((f0b > 0).double().mean()) < 0.9
    n = x.shape[1]
    need = engine.workspace_bytes(n, opts=opts)
    assert need >= engine.workspace_bytes(n, opts=engine.pipeline_opts(protect=0.33)) > 0
    arena = torch.empty(need, dtype=torch.uint8, device=engine.device)
    try:
        engine.set_workspace(arena)
        out = engine.pipeline_ex(x[0], opts, seed=3).cpu()
        assert 0 < engine.workspace_info()[2] <= need
        assert torch.equal(out, singles[0])
    finally:
        engine.set_workspace(None)
