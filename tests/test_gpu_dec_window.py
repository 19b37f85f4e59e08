"""The generator's output window (rvcx_set_dec_window, include/rvcx_test.h): the pipelines and the stream groups run the
HiFi-GAN generator only over the frames whose samples their trim keeps, plus the generator's receptive field.

Every case runs twice on the same context, input, seed and injected noise, window on and off, and the bar is
torch.equal on the whole returned tensor: the window removes work, it never changes a sample. The shapes are small
on purpose: at 350 frames nearly every decoder conv is split over K with a split count that depends on the tile count,
so a launch planned for the cropped length instead of the full one (ConvArgs::plan_T) takes another summation order
and fails the first case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UPP, I = 480, 192
N1 = 24000  # the first case: 24000 + 2 x 16000 samples -> 350 frames of audio, 348 of HuBERT features


def _frames(n, t_pad):
    """Frames of one chunk of n samples: min(len // 160, 2 L), L HuBERT's rows (vc_forward)."""
    m = n + 2 * t_pad
    return min(m // 160, 2 * ((m - 400) // 320 + 1))


def _audio(n, seed=7, B=None):
    from rvcx import synthetic

    if B is None:
        return synthetic.speech_like(n, seed=seed).astype(np.float64)
    return np.stack([synthetic.speech_like(n, seed=seed + b).astype(np.float64) for b in range(B)])


def _noise(frames, seed, B=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    lead = () if B is None else (B,)
    return (rng.standard_normal(lead + (I * frames,)).astype(np.float32),
            rng.standard_normal(lead + (frames * UPP,)).astype(np.float32))


def _window_frames(engine, T, t_pad_tgt):
    """The frames the generator runs on for the window [t_pad_tgt, T upp - t_pad_tgt) (dec_window_frames)."""
    M = engine.dec_margin_frames()
    s0, s1 = t_pad_tgt, T * UPP - t_pad_tgt
    fa, fb = max(0, s0 // UPP - M), min(T, -(-s1 // UPP) + M)
    return (fa, fb) if T - (fb - fa) >= 4 else (0, T)


@pytest.fixture()
def both(engine):
    """run(fn) -> (fn() with the window on, fn() with it off); the session engine gets its default back."""
    engine.set_pipeline_highpass()

    def run(fn):
        try:
            engine.set_dec_window(True)
            on = fn()
            torch.cuda.synchronize()
            on = [v.clone() for v in on] if isinstance(on, (tuple, list)) else on.clone()
            engine.set_dec_window(False)
            off = fn()
            torch.cuda.synchronize()
            off = [v.clone() for v in off] if isinstance(off, (tuple, list)) else off.clone()
        finally:
            engine.set_dec_window(True)
        engine.check_device_status()
        return on, off

    return run


@pytest.mark.parametrize("t_pad_tgt", [48000, 47999, 48001, 2400, 0])
def test_single_chunk(engine, both, t_pad_tgt):
    """48000: 100 frames trimmed per side, 90 dropped; 47999 / 48001: the window's edges fall inside a frame (floor at
    the start, ceil at the end); 2400 and 0: the margin swallows the trim and the generator runs full-length."""
    T = _frames(N1, 16000)
    fa, fb = _window_frames(engine, T, t_pad_tgt)
    assert (fb - fa < T) == (t_pad_tgt >= 47999)
    ez, es = _noise(T, 11)
    opts = engine.pipeline_opts(t_pad=16000, t_pad_tgt=t_pad_tgt)
    audio = _audio(N1)
    on, off = both(lambda: engine.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=3))
    assert on.shape == off.shape == (T * UPP - 2 * t_pad_tgt,)
    assert torch.isfinite(off).all() and float(off.abs().max()) > 0
    assert torch.equal(on, off)


def test_volume_envelope(engine, both):
    """volume_envelope != 1: the trim is a copy and the RMS envelope reads the kept samples (the non-fused path)."""
    T = _frames(N1, 16000)
    ez, es = _noise(T, 12)
    opts = engine.pipeline_opts(t_pad=16000, t_pad_tgt=48000, volume_envelope=0.5)
    audio = _audio(N1, seed=8)
    on, off = both(lambda: engine.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=4))
    assert on.shape == (T * UPP - 96000,) and torch.equal(on, off)


def test_multi_chunk(engine, both):
    """64000 samples with t_max 40000, t_center 32000, t_query 8000: one split point in [24000, 40000], two chunks of
    >= 350 frames, each with its own window. Both plans give 398 kept frames (each chunk loses its odd HuBERT row),
    so the split shows in the samples instead: the second chunk reads its noise at another offset and sees other
    HuBERT context than the unsplit run, whose output an unsplit second run would repeat bit for bit."""
    n = 64000
    ez, es = _noise(900, 13)  # more than both chunks draw
    audio = _audio(n, seed=9)
    one = engine.pipeline_ex(audio, engine.pipeline_opts(t_pad=16000, t_pad_tgt=48000), eps_z=ez, eps_src=es,
                             seed=5).clone()
    assert one.numel() == _frames(n, 16000) * UPP - 96000
    opts = engine.pipeline_opts(t_pad=16000, t_pad_tgt=48000, t_max=40000, t_center=32000, t_query=8000)
    on, off = both(lambda: engine.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=5))
    assert not torch.equal(off, one), "the input was not split"
    assert on.shape == off.shape and torch.equal(on, off)


def test_pipeline_batch(engine, both):
    """B = 3 rows share one window; every decoder launch takes the batch strides of the full-length buffers."""
    B, T = 3, _frames(N1, 16000)
    ez, es = _noise(T, 14, B)
    opts = engine.pipeline_opts(t_pad=16000, t_pad_tgt=48000)
    audio = _audio(N1, seed=20, B=B)
    on, off = both(lambda: engine.pipeline_batch(audio, opts, sids=[0, 1, 2], eps_z=ez, eps_src=es, seed=6))
    assert on.shape == off.shape == (B, T * UPP - 96000)
    assert torch.equal(on, off)
    assert not torch.equal(off[0], off[1])


def _stream_run(engine, window, opts_kw):
    """2 streams x 3 hops at the realtime benchmark's settings -> per hop (out, vol, offs)."""
    from rvcx import synthetic
    from rvcx.realtime import StreamGroup

    B, hops = 2, 3
    engine.set_dec_window(window)
    grp = StreamGroup(engine, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=[0, 1])
    try:
        block, T = grp.geometry["block48"], grp.geometry["frames"]
        assert (block, T) == (12288, 87)
        x = np.stack([synthetic.speech_like(block * hops, seed=40 + b, sr=48000).astype(np.float32) for b in range(B)])
        rng = np.random.Generator(np.random.PCG64(15))
        res = []
        for h in range(hops):
            ez = rng.standard_normal((B, I, T)).astype(np.float32)
            es = rng.standard_normal((B, T * UPP)).astype(np.float32)
            opts = [grp.opts(index_rate=0.0, **kw) for kw in opts_kw]
            out, vol = grp.process(x[:, h * block:(h + 1) * block], opts, eps_z=ez, eps_src=es, seed=h)
            torch.cuda.synchronize()
            res.append((out.clone(), vol.clone(), grp.offs.clone()))
        engine.check_device_status()
        return res, grp.geometry
    finally:
        grp.close()
        engine.set_dec_window(True)


@pytest.mark.parametrize("opts_kw", [({}, {"f0_up_key": 5}), ({}, {"volume_envelope": 0.5})],
                         ids=["windowed", "rms_row_full_length"])
def test_streams(engine, opts_kw):
    """The hop reads the first sola_search + block + crossfade samples of the model's output (17568 of 41760 here):
    output, SOLA offsets and vol equal with the window on and off. A row with a volume envelope makes the whole hop
    run full-length (the RMS envelope reads every sample): trivially equal."""
    on, geo = _stream_run(engine, True, opts_kw)
    off, _ = _stream_run(engine, False, opts_kw)
    assert geo["sola_search48"] + geo["block48"] + geo["crossfade48"] < geo["frames"] * UPP
    assert any(float(o[0].abs().max()) > 0 for o in off)
    for h, (a, b) in enumerate(zip(on, off)):
        for name, u, v in zip(("out", "vol", "offs"), a, b):
            assert torch.equal(u, v), (h, name)


def test_window_removes_work(engine):
    """Not vacuous: with kernel timing on, the first case's algorithmic FLOPs fall by the generator's FLOPs (measured
    on the generator alone at the same length) x the share of frames the window drops, within 3 % (the full-length
    noise conv of the first stage and the speaker-conditioning GEMM do not scale: < 0.1 % of the generator)."""
    T = _frames(N1, 16000)
    fa, fb = _window_frames(engine, T, 48000)
    ez, es = _noise(T, 11)
    opts = engine.pipeline_opts(t_pad=16000, t_pad_tgt=48000)
    audio = _audio(N1)
    engine.set_pipeline_highpass()
    rng = np.random.Generator(np.random.PCG64(16))
    z = rng.standard_normal((1, I, T)).astype(np.float32)
    f0 = np.full((1, T), 220.0, dtype=np.float32)
    fl = {}
    try:
        engine.profile(True)
        for on in (True, False):
            engine.set_dec_window(on)
            engine.profile_read()
            engine.pipeline_ex(audio, opts, eps_z=ez, eps_src=es, seed=3)
            torch.cuda.synchronize()
            fl[on] = engine.profile_read()[1]
        engine.dec_only(z, f0, [0], eps_src=es)
        torch.cuda.synchronize()
        dec = engine.profile_read()[1]
    finally:
        engine.profile(False)
        engine.set_dec_window(True)
    want = dec * (1.0 - (fb - fa) / T)
    print(f"\nframes {fb - fa} of {T}; GFLOP window on {fl[True] / 1e9:.2f}, off {fl[False] / 1e9:.2f}, generator alone "
          f"{dec / 1e9:.2f}; saved {(fl[False] - fl[True]) / 1e9:.2f}, expected {want / 1e9:.2f}")
    assert fl[True] < fl[False]
    assert abs((fl[False] - fl[True]) / want - 1.0) < 0.03


def test_margin_from_config(engine):
    """The margin is derived from the configuration: 10 frames for the 48 kHz v2 generator, more with a fourth
    dilation in every ResBlock, fewer with the widest kernel gone."""
    import dataclasses

    from rvcx.config import SYNTH_48K_V2

    assert engine.dec_margin_frames(SYNTH_48K_V2) == 10 == engine.dec_margin_frames()
    wider = dataclasses.replace(SYNTH_48K_V2, resblock_dilation_sizes=tuple(
        tuple(d) + (7,) for d in SYNTH_48K_V2.resblock_dilation_sizes))
    assert engine.dec_margin_frames(wider) > 10
    narrow = dataclasses.replace(SYNTH_48K_V2, resblock_kernel_sizes=tuple(SYNTH_48K_V2.resblock_kernel_sizes)[:2],
                                 resblock_dilation_sizes=tuple(SYNTH_48K_V2.resblock_dilation_sizes)[:2])
    assert engine.dec_margin_frames(narrow) < 10
