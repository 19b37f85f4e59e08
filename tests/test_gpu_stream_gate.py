"""The noise gate inside the realtime hop (rvcx_rt_set_clean per stream, carried by StreamGroup's options;
rvc/realtime/core.py:86-94, rvc/realtime/pipeline.py:326-327): where it sits, that it is per stream, and that it leaves the rest of the hop alone.

The kernels themselves are held to float64 in test_gpu_spectral_gate.py; here every comparison is between two device
runs and the bar is bit equality: the hop's gated rows against rvcx_spectral_gate on the rows the gate read
(rvcx_rt_model_rows, include/rvcx_test.h), the rows it read against a group that does not clean and runs its generator
full-length, and streams that do not clean against themselves. Geometry of the existing stream tests (read_chunk_size
96 -> 87 frames, 12288-sample blocks, 41760-sample model rows at 48 kHz); noise is injected and indexed by slot."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK, FRAMES = 12288, 87
RVCX_E_INVALID = -1


def _group(eng, B, **kw):
    from rvcx.realtime import StreamGroup

    grp = StreamGroup(eng, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=list(range(B)), **kw)
    assert grp.geometry["block48"] == BLOCK and grp.geometry["frames"] == FRAMES
    return grp


def _blocks(n, seed):
    from rvcx import synthetic

    return synthetic.speech_like(BLOCK * n, seed=seed, sr=48000).astype(np.float32).reshape(n, BLOCK)


def _noise(rng, B, cfg):
    return (rng.standard_normal((B, cfg.inter_channels, FRAMES)).astype(np.float32),
            rng.standard_normal((B, FRAMES * cfg.upp)).astype(np.float32))


def _hop(grp, x, opts, ez, es, active=None):
    out, _ = grp.process(x, opts, eps_z=ez, eps_src=es, active=active)
    torch.cuda.synchronize()
    return out.clone()


def _rows(eng, grp, n_active):
    """(the rows the gate read, the rows it left) of the group's last hop."""
    return eng.rt_model_rows(grp, n_active, False).clone(), eng.rt_model_rows(grp, n_active, True).clone()


def test_two_groups(engine):
    """Two 2-stream groups on the same audio and noise over three hops, one cleaning at 0.7."""
    from rvcx.config import SYNTH_48K_V2

    B, hops = 2, 3
    audio = np.stack([_blocks(hops, 120 + b) for b in range(B)])
    rng = np.random.default_rng(23)
    noise = [_noise(rng, B, SYNTH_48K_V2) for _ in range(hops)]
    C, P = _group(engine, B, clean_audio=True, clean_strength=0.7), _group(engine, B)
    oc, op = C.opts(index_rate=0.0), P.opts(index_rate=0.0)
    assert (oc.clean_audio, oc.clean_strength, op.clean_audio) == (1, 0.7, 0)
    for h in range(hops):
        yc = _hop(C, audio[:, h], oc, *noise[h])
        read, left = _rows(engine, C, B)
        if h == 0:  # the cleaning group's generator ran full-length and nothing before the gate moved
            engine.set_dec_window(False)
            try:
                yp = _hop(P, audio[:, h], op, *noise[h])
                plain, plain_left = _rows(engine, P, B)
            finally:
                engine.set_dec_window(True)
            assert torch.equal(read, plain) and torch.equal(plain, plain_left)
        else:
            yp = _hop(P, audio[:, h], op, *noise[h])
        assert read.shape == (B, FRAMES * SYNTH_48K_V2.upp)
        want = engine.spectral_gate(read, 48000, 0.7)
        assert torch.equal(left[:, : want.shape[1]], want), f"hop {h}"
        assert not left[:, want.shape[1]:].any()
        assert torch.isfinite(yc).all() and not torch.equal(yc, yp), f"hop {h}: the option is not live"
    C.close()
    P.close()


def test_three_slots(engine):
    """Strengths {0.3, off, 1.0}, the third slot idle on the second hop: the slot that does not clean keeps its rows
    bit for bit, and the idle slot gets zeros and its next hop is the one it would have had without the pause."""
    from rvcx.config import SYNTH_48K_V2

    B = 3
    audio = np.stack([_blocks(3, 130 + b) for b in range(B)])
    rng = np.random.default_rng(29)
    noise = [_noise(rng, B, SYNTH_48K_V2) for _ in range(3)]
    X, Y = _group(engine, B), _group(engine, B)
    strengths = [0.3, -1.0, 1.0]

    def opts(g):
        return [g.opts(index_rate=0.0, clean_audio=s >= 0, clean_strength=max(s, 0.0)) for s in strengths]

    nan = np.full(BLOCK, np.nan, np.float32)
    outs = []
    for h in range(3):
        x = audio[:, h].copy()
        active = None
        if h == 1:
            x[2] = nan
            active = [True, True, False]
        outs.append(_hop(X, x, opts(X), *noise[h], active=active))
        n_act = 2 if h == 1 else 3
        read, left = _rows(engine, X, n_act)
        assert torch.equal(left[1], read[1]), f"hop {h}: the slot that does not clean was touched"
        want = engine.spectral_gate(read, 48000, strengths[:n_act])
        assert torch.equal(left[:, : want.shape[1]], want), f"hop {h}"
        assert not torch.equal(left[0], read[0])
    assert not outs[1][2].any() and torch.isfinite(outs[1][:2]).all()
    # Y never saw the pause: its second hop is X's third for slot 2 (three active rows, the slot in the same position)
    _hop(Y, audio[:, 0], opts(Y), *noise[0])
    y2 = _hop(Y, audio[:, 2], opts(Y), *noise[2])
    assert torch.equal(y2[2], outs[2][2]) and outs[2][2].any()
    X.close()
    Y.close()


def test_40k(hubert_w, rmvpe_w):
    """One hop of a 40 kHz synthesizer (13 x 15 filter, the output resampler behind the gate)."""
    from rvcx.engine import Engine
    from synth_configs import CONFIGS, weights_for

    cfg = CONFIGS["v2_40k"]
    eng = Engine(0)
    try:
        eng.load_synth(weights_for("v2_40k"), cfg)
        eng.load_hubert(hubert_w)
        eng.load_rmvpe(rmvpe_w)
        B = 2
        grp = _group(eng, B, clean_audio=True, clean_strength=0.5)
        audio = np.stack([_blocks(1, 140 + b)[0] for b in range(B)])
        ez, es = _noise(np.random.default_rng(31), B, cfg)
        out = _hop(grp, audio, grp.opts(index_rate=0.0), ez, es)
        read, left = _rows(eng, grp, B)
        assert read.shape == (B, FRAMES * 400)
        want = eng.spectral_gate(read, 40000, 0.5)
        assert want.shape == (B, 256 * (FRAMES * 400 // 256))
        assert torch.equal(left[:, : want.shape[1]], want) and not torch.equal(left, read)
        assert torch.isfinite(out).all() and out.any()
        grp.close()
    finally:
        eng.close()


def test_errors(engine):
    from rvcx import _lib
    from rvcx.realtime import StreamGroup, VoiceChanger

    grp = _group(engine, 1)
    with pytest.raises(ValueError):
        grp.opts(clean_strength=1.5)
    with pytest.raises(ValueError):
        _group(engine, 1, clean_strength=-0.5)
    # options filled in by hand are refused before the hop; the library refuses the same by itself, changes no
    # setting, and the group goes on as a fresh one does
    bad = grp.opts(index_rate=0.0, clean_audio=True)
    bad.clean_strength = 1.5
    x = _blocks(1, 150)
    ez, es = _noise(np.random.default_rng(37), 1, engine.synth_cfg)
    with pytest.raises(ValueError):
        grp.process(x, bad, eps_z=ez, eps_src=es)
    lib = engine.lib
    assert lib.rvcx_rt_set_clean(engine.ctx, grp.handle, 0, 1, 1.5) == RVCX_E_INVALID
    assert lib.rvcx_rt_set_clean(engine.ctx, grp.handle, 0, 1, float("nan")) == RVCX_E_INVALID
    assert lib.rvcx_rt_set_clean(engine.ctx, grp.handle, 1, 1, 0.5) == RVCX_E_INVALID  # a 1-stream group
    assert lib.rvcx_rt_set_clean(engine.ctx, grp.handle, -1, 0, 0.0) == 0  # every stream off: what it was
    fresh = _group(engine, 1)
    good = grp.opts(index_rate=0.0, clean_audio=True, clean_strength=0.5)
    assert torch.equal(_hop(grp, x, good, ez, es), _hop(fresh, x, good, ez, es))
    grp.close()
    fresh.close()
    # read_chunk_size 97 without extra context: the model row is 17760 samples, the gate returns 17664 of them and
    # SOLA reads up to sample 17695
    tight = StreamGroup(engine, 1, read_chunk_size=97, cross_fade_overlap_size=0.1, extra_convert_size=0.0,
                        silent_threshold=-90.0)
    assert tight.geometry["frames"] == 37
    xt = np.zeros((1, 97 * 128), np.float32)
    with pytest.raises(_lib.RvcxError) as e:
        tight.process(xt, tight.opts(index_rate=0.0, clean_audio=True))
    assert e.value.code == RVCX_E_INVALID and "tail" in str(e.value)
    tight.close()
    with pytest.raises(ValueError, match="post_process"):
        VoiceChanger(96, 0.1, 0.5, engine=engine, post_process=True)
    with pytest.raises(ValueError, match="vad_enabled"):
        VoiceChanger(96, 0.1, 0.5, engine=engine, vad_enabled=True)
    with pytest.raises(ValueError):
        VoiceChanger(96, 0.1, 0.5, engine=engine, clean_audio=True, clean_strength=2)


def test_voice_changer(engine):
    """VoiceChanger(clean_audio=True) as in the reference: the first hop's output differs from clean_audio=False."""
    from rvcx.realtime import VoiceChanger

    x = _blocks(1, 160)[0]
    outs = []
    for clean in (False, True):
        vc = VoiceChanger(96, 0.1, 0.5, engine=engine, silent_threshold=-90, clean_audio=clean, clean_strength=0.5,
                          model_path="unused.pth", vad_sensitivity=3)
        out, vol, _ = vc.on_request(x.copy(), index_rate=0.0)
        assert out.shape == (BLOCK,) and np.isfinite(out).all() and vol > 0
        outs.append(out)
        vc.close()
    assert outs[0].any() and not np.array_equal(outs[0], outs[1])
