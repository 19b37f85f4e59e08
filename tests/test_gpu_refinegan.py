"""The RefineGAN decoder (csrc/runtime_refinegan.cpp, csrc/refinegan.hip) on the device against the oracle in float64, at
48, 40 and 32 kHz (rg_48k / rg_40k / rg_32k: the v2 upsample lists with vocoder="RefineGAN", seeded weights), and MRF
HiFi-GAN beside 48 kHz. Every bar is K = 8 gaps of the CPU oracle's own fp32-vs-fp64 distance on the test's inputs
(tests/parity_anchor.py; (K + 1) against a stored fp32 fixture) or a bar of the file it is cited from; no number is
tuned to the device. tests/test_refinegan_cpu.py shows which decoder mistakes the K-gap bar catches.

  1. Synthesizer.infer at lengths (24, 17, 1), sids (3, 0, 108): all five outputs in chain order, every T upp sample of
     every row (the reference runs the decoder on z * mask over all T frames);
  2. the generator alone on the oracle's z at T = 1 and 2 (every resample stage clamps on both sides: the coarsest reads
     r0 T rows through 2 width + r0 taps) and, at 32 kHz, T = 137 (odd, 43 840 samples); the kernel families the
     rg_48k call launched must each be the policy family of an rg.* row of tests/conv_form_ref.py;
  3. the second pin to the reference's own run (tests/golden/synth_refinegan_b3_40k.npz);
  4. seeded noise (eps_src = None), and the five-stage list refused at finalize;
  5. the decoder inside the pipeline (output window on == off), the ragged batch and a stream group.
"""
import numpy as np
import pytest
import torch

import parity_anchor as pa
import refinegan_ref as rr
import synth_configs as sc
from conftest import golden, refinegan_noise
from parity_anchor import K, anchor, anchored, check, check_each

pytestmark = pytest.mark.gpu

RG = ("rg_48k", "rg_40k", "rg_32k")


@pytest.fixture(scope="module")
def engines(hubert_w, rmvpe_w):
    """get(name, vocoder, front) -> (name, cfg, weights, Engine): one Engine per (configuration, decoder), made at its
    first use; HuBERT and RMVPE are loaded when a whole-path test first asks (front)."""
    from rvcx.engine import Engine

    made = {}

    def get(name, vocoder="RefineGAN", front=False):
        key = (name, vocoder)
        cfg, w = rr.config(name, vocoder), rr.weights_for(name, vocoder)
        if key not in made:
            e = Engine(0)
            e.load_synth(w, cfg)
            assert e.upp == cfg.upp == cfg.sr // 100
            made[key] = [e, False]
        if front and not made[key][1]:
            made[key][0].load_hubert(hubert_w)
            made[key][0].load_rmvpe(rmvpe_w)
            made[key][1] = True
        return name, cfg, w, made[key][0]

    yield get
    for e, _ in made.values():
        e.close()


# ----------------------------------------------------------------- 1. the synthesizer chain
def _synth_vs_fp64(name, cfg, w, eng, c):
    assert tuple(c["sid"]) == pa.SIDS and not c["f0"][-1].any() and tuple(c["lengths"]) == rr.LENGTHS
    anc = anchor(pa.synth_fn(w, cfg=cfg, **c))
    out = eng.synth_infer_ex(c["phone"], c["lengths"], c["pitch"], c["f0"], c["sid"], eps_z=c["eps_z"],
                             eps_src=c["eps_src"])
    eng.check_device_status()
    dev = dict(zip(("o", "z_p", "z", "m_p", "logs_p"), (eng.host(v) for v in out)))
    assert dev["o"].shape == (3, rr.LENGTHS[0] * cfg.upp)
    check_each([(f"{name} synth {rr.LENGTHS} {k}", dev[k], *anc[k], K) for k in ("m_p", "logs_p", "z_p", "z", "o")])


@pytest.mark.parametrize("name", RG)
def test_synth_vs_fp64(engines, name):
    name, cfg, w, eng = engines(name)
    c = rr.synth_case(cfg)
    from oracle.synth import refinegan_noise_sizes

    assert c["eps_src"].size == sum(refinegan_noise_sizes(cfg, 3, 24))
    _synth_vs_fp64(name, cfg, w, eng, c)


@pytest.mark.parametrize("name", ["rg_40k", "rg_32k"])
def test_mrf_synth_vs_fp64(engines, name):
    """MRF HiFi-GAN beside 48 kHz: the same (24, 17, 1) anchor on the 40 and 32 kHz lists (eps_src: [B][N][9] randn,
    then [B][9] U(0, 1) initial phases)."""
    _, cfg, w, eng = engines(name, "MRF HiFi-GAN")
    c = pa.synth_case(rr.LENGTHS, rr.SEED, cfg=cfg)
    rng = np.random.Generator(np.random.PCG64(rr.SEED + 1))
    n = 3 * 24 * cfg.upp * 9
    c["eps_src"] = np.concatenate([rng.standard_normal(n), rng.random(3 * 9)]).astype(np.float32)
    _synth_vs_fp64(name.replace("rg", "mrf"), cfg, w, eng, c)


# ----------------------------------------------------------------- 2. the generator alone
def _oracle_z(w, cfg, c):
    """The oracle's fp32 z [B, I, T] of a synth case (TextEncoder -> flow reverse), without its decoder."""
    import torch.nn.functional as F

    from oracle import synth as osynth

    t = torch.from_numpy
    with torch.no_grad():
        g = F.embedding(t(c["sid"]), osynth._t(w, "emb_g.weight")).unsqueeze(-1)
        m_p, logs_p, mask = osynth.text_encoder(w, cfg, t(c["phone"]), t(c["pitch"]), t(c["lengths"]))
        z_p = (m_p + torch.exp(logs_p) * t(c["eps_z"]) * 0.66666) * mask
        return osynth.flow_reverse(w, cfg, z_p, mask, g).numpy()


DEC = [(n, T) for n in RG for T in (1, 2)] + [("rg_32k", 137)]


@pytest.mark.parametrize("name,T", DEC, ids=[f"{n}-T{T}" for n, T in DEC])
def test_dec_only_vs_fp64(engines, name, T):
    import conv_form_ref as cf

    RG_POLICY = cf.RG_POLICY
    name, cfg, w, eng = engines(name)
    c = pa.synth_case((T,), 40 + T, cfg=cfg)
    z = _oracle_z(w, cfg, c)
    es = rr.noise(cfg, 1, T, np.random.Generator(np.random.PCG64(50 + T)))
    ref, gap = anchor(pa.dec_fn(w, z, c["f0"], c["sid"], es, cfg=cfg))["out"]
    probe = (name, T) == ("rg_48k", 2)
    try:
        if probe:
            eng.profile(True)
            eng.profile_read_kinds()
        o = eng.dec_only(z, c["f0"], c["sid"], eps_src=es)
        torch.cuda.synchronize()
        fam = eng.profile_read_kinds()[1] if probe else {}
    finally:
        if probe:
            eng.profile(False)
    eng.check_device_status()
    assert o.shape == (1, T * cfg.upp)
    check(f"{name} dec_only (1, {T})", eng.host(o), ref, gap, K)
    if probe:
        ran = {k for k, v in fam.items() if v["launches"] > 0 and k.startswith("conv_")}
        print(f"\n{name} dec_only T={T} kernel families: " +
              ", ".join(f"{k} x{v['launches']}" for k, v in sorted(fam.items()) if v["launches"] > 0))
        assert {c["name"] for c in cf.CASES if c["name"].startswith("rg.")} == set(RG_POLICY)
        assert ran and ran <= set(RG_POLICY.values()), sorted(ran - set(RG_POLICY.values()))


# ----------------------------------------------------------------- 3. the second pin to the reference's own run
def test_refinegan_b3_40k_vs_reference(engines):
    """tests/golden/synth_refinegan_b3_40k.npz (make_golden_vocoders.py refinegan_b3_40k): the reference's own
    Synthesizer(vocoder="RefineGAN").infer on the 40 kHz list, B = 3, lengths (24, 17, 1). The fixture within 2 gaps
    of float64, the device within (K + 1) gaps of the fixture and K of float64."""
    from rvcx import synthetic
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state

    g = golden("synth_refinegan_b3_40k.npz")
    cfg = rr.config("rg_40k")
    w = normalize_state(synthetic.synth_state(int(g["seed_w"]), cfg))
    eps_z, eps_src = refinegan_noise(g)
    B, T = g["phone"].shape[:2]
    eps_z = eps_z.reshape(B, cfg.inter_channels, T)
    eng = Engine(0)
    try:
        eng.load_synth(w, cfg)
        out, zp, z = eng.synth_infer(g["phone"], g["lengths"], g["pitch"], g["f0"], g["sid"], eps_z=eps_z,
                                     eps_src=eps_src, want_latents=True)
        torch.cuda.synchronize()
        eng.check_device_status()
        o, z = out.cpu().numpy(), z.cpu().numpy()
    finally:
        eng.close()
    anc = anchor(pa.synth_fn(w, g["phone"], g["lengths"], g["pitch"], g["f0"], g["sid"], eps_z, eps_src, cfg=cfg))
    check_each([(f"synth_refinegan_b3_40k {k} device vs fp64", v, *anc[k], K) for k, v in (("z", z), ("o", o))])
    anchored("synth_refinegan_b3_40k z", z, g["z"].transpose(0, 2, 1), *anc["z"], 1e-4)
    anchored("synth_refinegan_b3_40k o", o, g["o"], *anc["o"], 2e-3)


# ----------------------------------------------------------------- 4. seeded noise; the refused list
def test_generated_noise_is_seeded(engines):
    """eps_src = None: the source and the 24 AdaIN draws come from Philox(seed) (normal_at in k_adain, nseed(k) per
    draw): same seed -> same output bit for bit, new seed -> new, finite (test_mrf_generated_noise_is_seeded)."""
    _, cfg, _, eng = engines("rg_40k")
    c = rr.synth_case(cfg)
    run = lambda seed: eng.synth_infer(c["phone"], c["lengths"], c["pitch"], c["f0"], c["sid"],  # noqa: E731
                                       eps_z=c["eps_z"], seed=seed).cpu().numpy()
    a, b, d = run(5), run(5), run(6)
    assert np.array_equal(a, b) and not np.array_equal(a, d) and np.isfinite(a).all() and np.isfinite(d).all()
    assert float(np.abs(a).max()) > 0


def test_five_stage_list_is_refused_at_finalize():
    """v1_48k (rates 10, 6, 2, 2, 2) with vocoder="RefineGAN": five doublings from 16 channels end the source branch at
    512, not the 256 the concat takes (the reference cannot run it either). RVCX_E_SHAPE at finalize, nothing loaded."""
    import dataclasses

    from rvcx import _lib, synthetic
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state
    from synth_configs import CONFIGS

    cfg = dataclasses.replace(CONFIGS["v1_48k"], vocoder="RefineGAN")
    e = Engine(0)
    try:
        with pytest.raises(_lib.RvcxError) as ei:
            e.load_synth(normalize_state(synthetic.synth_state(1, cfg)), cfg)
        assert ei.value.code == -2 and _lib.STATUS[-2] == "RVCX_E_SHAPE", ei.value
        assert not e.loaded["synth"]
    finally:
        e.close()


# ----------------------------------------------------------------- 5. the decoder inside the whole paths
@pytest.fixture(scope="module")
def clip(rmvpe_w):
    """test_gpu_synth_configs.clip: the 2.5 s clip and the oracle's own fp32 salience gap on its padded input."""
    from scipy import signal

    from oracle.pipeline import AH, BH

    audio = golden("pipeline_2p5s.npz")["audio"].astype(np.float64)
    x = np.pad(signal.filtfilt(BH, AH, audio), (16000, 16000), mode="reflect")
    _, gap = anchor(pa.rmvpe_fn(rmvpe_w, x.astype(np.float32)[None]))["out"]
    return audio, gap


@pytest.mark.parametrize("name", ["rg_48k", "rg_40k"])
def test_pipeline_vs_oracle_and_window(engines, clip, hubert_w, rmvpe_w, name):
    """test_gpu_synth_configs.pipeline_vs_oracle (its decomposition and bars) with this decoder: one chunk, so one
    src_noise_total(1, T) block. Then the output window on and off on the same inputs: torch.equal and full length
    (runtime.h: "MRF and RefineGAN ignore the window")."""
    from oracle.synth import src_noise_floats

    name, cfg, w, eng = engines(name, front=True)
    audio, ez, es, out = sc.pipeline_vs_oracle((name, cfg, w, eng), clip, hubert_w, rmvpe_w)
    T = ez.size // cfg.inter_channels
    assert es.size == src_noise_floats(cfg, 1, T) and out.shape == (T * cfg.upp - 2 * cfg.sr,)
    opts = eng.pipeline_opts(protect=0.33, t_pad=16000, t_pad_tgt=cfg.sr)
    res = {}
    try:
        for on in (True, False):
            eng.set_dec_window(on)
            res[on] = eng.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=3).clone()
            torch.cuda.synchronize()
    finally:
        eng.set_dec_window(True)
    eng.check_device_status()
    assert res[True].shape == res[False].shape == (T * cfg.upp - 2 * cfg.sr,)
    assert torch.isfinite(res[False]).all() and float(res[False].abs().max()) > 0
    assert torch.equal(res[True], res[False])


def batch_noise(cfg, B, T, rng):
    """A ragged batch's injected noise: eps_z [B, I, T] and the decoder's flat blocks for B rows of T frames."""
    return rng.standard_normal((B, cfg.inter_channels, T)).astype(np.float32), rr.noise(cfg, B, T, rng)


def test_ragged_batch_matches_single(engines):
    """Rows n = 24000 / 40000 / 8000 through pipeline_batch_v against rvcx_pipeline_ex per row, each single call with
    its row's noise cut out of the batch's [B][C][T_stage] blocks (refinegan_ref.row_noise), at the bars of
    tests/test_gpu_ragged_batch.py check_rows_vs_single: equal shape, spectrogram correlation > 0.999, max difference
    < 5e-3 of the peak, the same f0 bit for bit. The batch runs the decoder on z * mask over the longest row's frames
    (as the reference's batched Synthesizer.infer would); what lies beyond a short row's end reaches back through the
    resamplers' taps, but on the oracle it is 1e-5 of the peak 10 frames before the end and 1e-6 at the 30 frames these
    options trim: far inside these bars."""
    from oracle.metrics import spectrogram_correlation
    from ragged_rows import SHORT_PAD
    from ragged_rows import clip as speech

    _, cfg, _, eng = engines("rg_48k", front=True)
    ns, sids = [24000, 40000, 8000], [0, 3, 7]
    audios = [speech(n, 90 + b) for b, n in enumerate(ns)]
    eng.set_pipeline_highpass()
    opts = eng.pipeline_opts(pitch=2.0, protect=0.33, **SHORT_PAD)
    Ts = [eng.pipeline_frames(n, opts) for n in ns]
    ez, es = batch_noise(cfg, len(ns), max(Ts), np.random.default_rng(3))
    ys, f0s = eng.pipeline_batch_v(audios, opts, sids=sids, eps_z=ez, eps_src=es, want_f0=True)
    ys, f0s = [eng.host(y) for y in ys], [eng.host(f) for f in f0s]
    failed = []
    for b, a in enumerate(audios):
        o1 = eng.pipeline_opts(pitch=2.0, protect=0.33, sid=sids[b], **SHORT_PAD)
        y1, f1 = eng.pipeline_ex(a, o1, eps_z=np.ascontiguousarray(ez[b, :, :Ts[b]]).reshape(-1),
                                 eps_src=rr.row_noise(cfg, es, len(ns), max(Ts), b, Ts[b]), want_f0=True)
        y1, f1 = eng.host(y1), eng.host(f1)
        assert ys[b].shape == y1.shape == (Ts[b] * cfg.upp - 2 * int(opts.t_pad_tgt),), (b, ys[b].shape, y1.shape)
        corr = spectrogram_correlation(ys[b], y1)
        diff = float(np.abs(ys[b] - y1).max()) / max(float(np.abs(y1).max()), 1e-6)
        print(f"\nrg_48k ragged row {b} n={ns[b]} T={Ts[b]}: corr {corr:.6f} max diff / peak {diff:.3e}")
        if not (corr > 0.999 and diff < 5e-3):
            failed.append(f"row {b}: corr {corr:.6f} diff {diff:.3e}")
        if not np.array_equal(f0s[b], f1):
            failed.append(f"row {b}: f0 differs from the single run's")
    eng.check_device_status()
    assert not failed, "; ".join(failed)


def test_stream_group_matches_oracle(engines, hubert_w, rmvpe_w):
    """test_gpu_synth_configs.stream_group_vs_oracle (B = 2, that test's bars) at 40 kHz with this decoder, two hops;
    the group takes the batch's blocks, each oracle stream its row's."""
    name, cfg, w, eng = engines("rg_40k", front=True)

    def src_noise(rng, B, T):
        es = rr.noise(cfg, B, T, rng)
        return es, [rr.row_noise(cfg, es, B, T, b)[None] for b in range(B)]

    sc.stream_group_vs_oracle((name, cfg, w, eng), hubert_w, rmvpe_w, hops=2, src_noise=src_noise)


def test_stream_group_refuses_injected_noise_with_an_idle_slot(engines):
    """runtime_stream.cpp: the rows of this decoder's injected source noise cannot be gathered by slot, so a hop with
    an idle slot and eps_src is RVCX_E_INVALID (with generated noise it runs)."""
    from rvcx import _lib
    from rvcx.realtime import StreamGroup

    _, cfg, _, eng = engines("rg_40k", front=True)
    grp = StreamGroup(eng, 2, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=[0, 1])
    try:
        T, block = grp.geometry["frames"], grp.geometry["block48"]
        x = np.zeros((2, block), np.float32)
        es = rr.noise(cfg, 2, T, np.random.default_rng(1))
        with pytest.raises(_lib.RvcxError) as e:
            grp.process(x, grp.opts(), eps_src=es, active=[True, False])
        assert e.value.code == -1 and _lib.STATUS[-1] == "RVCX_E_INVALID", e.value
        out, _ = grp.process(x, grp.opts(), seed=1, active=[True, False])
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
    finally:
        grp.close()
