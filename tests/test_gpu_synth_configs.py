"""The synthesizer configurations beside SYNTH_48K_V2 on the device (tests/synth_configs.py: the 40 kHz and 32 kHz v2
models and two five-stage v1 lists) against the oracle in float64. The rule: a configuration rvcx_set_synth_config +
rvcx_finalize accept yields the float64 answer within the project's bar, K = 8 times the oracle's own fp32-vs-fp64 gap
on the same inputs (tests/parity_anchor.py); one the kernels cannot serve is refused with RVCX_E_SHAPE at finalize.

  1. every output of Synthesizer.infer (m_p, logs_p, z_p, z, waveform) at lengths (24, 17, 1), sids (3, 0, 108);
  2. the generator alone at B = 1, T = 840, where the second up-conv's tile policy changes (pick_wsb: plan_rows >=
     8192, with u0 = 10 from T = 820), with the kernel families the call ran;
  3. the output window (rvcx_set_dec_window) on and off, bit for bit, with the configuration's margin and upp;
  4. the whole pipeline at t_pad_tgt = cfg.sr against the oracle pipeline, decomposed as tests/test_gpu_sizes.py
     does it, for v2_40k and for v1_32k (HuBERT final_proj -> 256-dim upsample / protect -> emb_phone);
  5. a stream group whose model is not 48 kHz (the second resample tgt_sr -> 48000) against OracleVoiceChanger.

Every anchored point prints `name: err bound err/gap`; tests/test_synth_configs_cpu.py shows which configuration
mistakes these bars catch. No number here is tuned to the device: each bar is K gaps of the CPU float64 oracle or a
bar of the file it is cited from.
"""
import numpy as np
import pytest
import torch

import parity_anchor as pa
from conftest import golden
from parity_anchor import K, anchor, check, check_each
from synth_configs import CONFIGS, NAMES, pipeline_vs_oracle, stream_group_vs_oracle, weights_for

pytestmark = pytest.mark.gpu

LENGTHS, SEED = (24, 17, 1), 7  # the point of tests/test_synth_configs_cpu.py
TWO = ("v2_40k", "v1_32k")  # one v2 configuration off 48 kHz, and the five-stage v1 one with the 5-tap up-conv


@pytest.fixture(scope="module")
def engines(hubert_w, rmvpe_w):
    """get(name) -> (name, cfg, weights, Engine): one Engine per configuration, made at its first use with the
    configuration's seeded synthesizer and the session's HuBERT / RMVPE, all closed when the module is done."""
    from rvcx.engine import Engine

    made = {}

    def get(name):
        if name not in made:
            cfg, w = CONFIGS[name], weights_for(name)
            e = made[name] = Engine(0)
            e.load_synth(w, cfg)
            e.load_hubert(hubert_w)
            e.load_rmvpe(rmvpe_w)
            assert e.upp == cfg.upp == cfg.sr // 100
        return name, CONFIGS[name], weights_for(name), made[name]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture()
def cfg_engine(engines, request):
    return engines(request.param)


def only(names):
    return pytest.mark.parametrize("cfg_engine", names, indirect=True)


# ----------------------------------------------------------------- 1. the synthesizer chain
@only(NAMES)
def test_synth_vs_fp64(cfg_engine):
    """test_gpu_module_fp64.test_synth_vs_fp64 per configuration: all five outputs in the order of the chain."""
    name, cfg, w, eng = cfg_engine
    c = pa.synth_case(LENGTHS, SEED, cfg=cfg)
    coarse = set(c["pitch"].reshape(-1).tolist())
    assert tuple(c["sid"]) == pa.SIDS and 255 in coarse and 1 in coarse and not c["f0"][-1].any()
    assert c["phone"].shape == (3, 24, cfg.text_enc_hidden_dim) and c["eps_src"].shape == (3, 24 * cfg.upp)
    anc = anchor(pa.synth_fn(w, cfg=cfg, **c))
    out = eng.synth_infer_ex(c["phone"], c["lengths"], c["pitch"], c["f0"], c["sid"], eps_z=c["eps_z"],
                             eps_src=c["eps_src"])
    dev = dict(zip(("o", "z_p", "z", "m_p", "logs_p"), (eng.host(v) for v in out)))
    check_each([(f"{name} synth {LENGTHS} {k}", dev[k], *anc[k], K) for k in ("m_p", "logs_p", "z_p", "z", "o")])


# ----------------------------------------------------------------- 2. the generator where the tile policy changes
@only(TWO)
def test_dec_only_t840_vs_fp64(cfg_engine):
    """B = 1, T = 840: the second up-conv plans 8400 rows, beyond pick_wsb's 8192. The weight-streamed and the
    weight-stationary families must both have run, so the length cannot go stale silently."""
    from rvcx import synthetic

    name, cfg, w, eng = cfg_engine
    T = 840
    rng = np.random.Generator(np.random.PCG64(63))
    z = rng.standard_normal((1, cfg.inter_channels, T)).astype(np.float32)
    f0 = synthetic.f0_walk(1, T, seed=63).astype(np.float32)
    f0[0, T // 3:T // 3 + 40] = 0.0  # an unvoiced run inside
    es = rng.standard_normal((1, T * cfg.upp)).astype(np.float32)
    ref, gap = anchor(pa.dec_fn(w, z, f0, [0], es, cfg=cfg))["out"]
    try:
        eng.profile(True)
        eng.profile_read_kinds()
        o = eng.dec_only(z, f0, [0], eps_src=es)
        torch.cuda.synchronize()
        _, fam = eng.profile_read_kinds()
    finally:
        eng.profile(False)
    print(f"\n{name} dec_only T={T} kernel families: " +
          ", ".join(f"{k} x{v['launches']}" for k, v in sorted(fam.items())))
    assert fam.get("conv_wsb16_kernel", {}).get("launches", 0) > 0, fam
    assert fam.get("conv_wst16_kernel", {}).get("launches", 0) > 0, fam
    check(f"{name} dec_only (1, {T})", eng.host(o), ref, gap, K)


# ----------------------------------------------------------------- 3. the output window
def _frames(n, t_pad):
    """Frames of one chunk of n samples: min(len // 160, 2 L), L HuBERT's rows (test_gpu_dec_window._frames)."""
    m = n + 2 * t_pad
    return min(m // 160, 2 * ((m - 400) // 320 + 1))


@only(NAMES)
@pytest.mark.parametrize("short", [0, 1], ids=["sr", "sr-1"])
def test_output_window(cfg_engine, short):
    """test_gpu_dec_window.test_single_chunk with the configuration's upp, sample rate and margin: 24000 samples,
    t_pad 16000, t_pad_tgt = cfg.sr (100 frames per side) and cfg.sr - 1 (the window's edges inside a frame), window
    on and off on the same context, input, seed and injected noise. Bar: torch.equal, that file's."""
    from rvcx import synthetic

    name, cfg, w, eng = cfg_engine
    N, upp, t_pad_tgt = 24000, cfg.upp, cfg.sr - short
    T = _frames(N, 16000)
    M = eng.dec_margin_frames()
    s0, s1 = t_pad_tgt, T * upp - t_pad_tgt
    fa, fb = max(0, s0 // upp - M), min(T, -(-s1 // upp) + M)
    assert T - (fb - fa) >= 4 and fb - fa < T, (fa, fb, T)  # the window drops frames (dec_window_frames)
    rng = np.random.Generator(np.random.PCG64(11))
    ez = rng.standard_normal((cfg.inter_channels * T,)).astype(np.float32)
    es = rng.standard_normal((T * upp,)).astype(np.float32)
    audio = synthetic.speech_like(N, seed=7).astype(np.float64)
    eng.set_pipeline_highpass()
    opts = eng.pipeline_opts(t_pad=16000, t_pad_tgt=t_pad_tgt)
    res = {}
    try:
        for on in (True, False):
            eng.set_dec_window(on)
            res[on] = eng.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=3).clone()
            torch.cuda.synchronize()
    finally:
        eng.set_dec_window(True)
    eng.check_device_status()
    on, off = res[True], res[False]
    print(f"\n{name} window t_pad_tgt={t_pad_tgt}: margin {M}, frames {fb - fa} of {T}")
    assert on.shape == off.shape == (T * upp - 2 * t_pad_tgt,)
    assert torch.isfinite(off).all() and float(off.abs().max()) > 0
    assert torch.equal(on, off)


# ----------------------------------------------------------------- 4. the pipeline at another target rate, v1 end to end
@pytest.fixture(scope="module")
def clip(rmvpe_w):
    """The 2.5 s clip of pipeline_2p5s.npz, the padded input the oracle's RMVPE sees, and how far the oracle's own
    fp32 salience sits from float64 on it (what the fixtures of test_gpu_sizes.py store as sal_fp32_noise)."""
    from scipy import signal

    from oracle.pipeline import AH, BH

    audio = golden("pipeline_2p5s.npz")["audio"].astype(np.float64)
    x = np.pad(signal.filtfilt(BH, AH, audio), (16000, 16000), mode="reflect")
    _, gap = anchor(pa.rmvpe_fn(rmvpe_w, x.astype(np.float32)[None]))["out"]
    return audio, gap


@only(TWO)
def test_pipeline_vs_oracle(cfg_engine, clip, hubert_w, rmvpe_w):
    pipeline_vs_oracle(cfg_engine, clip, hubert_w, rmvpe_w)


# ----------------------------------------------------------------- 5. streaming with a model that is not 48 kHz
@only(("v2_40k",))
def test_stream_group_matches_oracle(cfg_engine, hubert_w, rmvpe_w):
    stream_group_vs_oracle(cfg_engine, hubert_w, rmvpe_w)


# ----------------------------------------------------------------- the other half of the rule: refused, never wrong
def test_unservable_configuration_is_refused_at_finalize():
    """Stage 0 with k = 17, u = 10: padding (k - u) // 2 = 3 makes the ConvTranspose give 10 T + 1 samples, a length
    the polyphase form (T rows of u phases) does not produce. rvcx_finalize refuses with RVCX_E_SHAPE and names the
    stage; nothing has run by then."""
    import dataclasses

    from rvcx import _lib, synthetic
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state

    cfg = dataclasses.replace(CONFIGS["v2_40k"], upsample_kernel_sizes=(17, 16, 4, 4))
    e = Engine(0)
    try:
        with pytest.raises(_lib.RvcxError) as ei:
            e.load_synth(normalize_state(synthetic.synth_state(1, cfg)), cfg)
        assert ei.value.code == -2 and _lib.STATUS[-2] == "RVCX_E_SHAPE", ei.value
        assert "stage 0" in str(ei.value), ei.value
        assert not e.loaded["synth"]
    finally:
        e.close()
