"""Realtime streams with f0_method "fcpe" on device: one batched FCPE forward per hop (rvcx_rt_desc.f0_method 1) in
place of the batched RMVPE, everything else of the hop unchanged.

The yardstick is the REFERENCE's own run (tests/golden/stream_fcpe_4.npz: rvc/realtime VoiceChanger(...,
f0_method="fcpe") for 4 streams x 4 hops with the seeded 2-layer FCPE model, made by
tests/golden/make_golden_stream_fcpe.py), at the bars of test_stream_group_16_matches_reference, unchanged: vol rel
<= 1e-5; gated hops: offset 0 and the crossfade tail; per-hop spectrogram correlation >= 0.999; max |diff| <= 2e-3 of
the hop's peak where the SOLA offset agrees; offsets equal on >= 95 % of the compared hops. Hops the fixture flags
"unsure" (a voiced frame whose peak bin could move out of the local_argmax window within the fp32 error bound) are
exempt from the waveform and offset bars only. tests/test_stream_fcpe_cpu.py asserts the fixture's conditions and
reproduces it with a CPU restatement."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from stream_fcpe_ref import hop_noise, stream_inputs

pytestmark = pytest.mark.gpu

GEOM = dict(read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5, silent_threshold=-90.0)


def _fcpe_weights(g):
    from rvcx import synthetic

    return (synthetic.fcpe_state(int(g["fcpe_seed"]), int(g["fcpe_layers"]), int(g["fcpe_chans"])),
            synthetic.fcpe_config(int(g["fcpe_layers"]), int(g["fcpe_chans"])))


@pytest.fixture(scope="module")
def fx(engine):
    """The fixture, its regenerated inputs, and the seeded FCPE model loaded into the session engine."""
    g = golden("stream_fcpe_4.npz")
    engine.load_fcpe(*_fcpe_weights(g))
    return dict(g=g, x=stream_inputs(g))


def _sizes(grp):
    from rvcx.config import SYNTH_48K_V2

    return SYNTH_48K_V2.inter_channels, grp.geometry["frames"], SYNTH_48K_V2.upp


def _rngs(g):
    return [np.random.Generator(np.random.PCG64(int(g["noise_seed0"]) + s)) for s in range(int(g["n_streams"]))]


def test_stream_group_fcpe_matches_reference(engine, fx):
    from oracle.metrics import spectrogram_correlation
    from rvcx.realtime import StreamGroup

    g, x = fx["g"], fx["x"]
    S, H, blk = int(g["n_streams"]), int(g["hops"]), int(g["block"])
    grp = StreamGroup(engine, S, sid=[int(v) for v in g["sids"]], f0_method="fcpe",
                      fcpe_threshold=float(g["threshold"]), **GEOM)
    geo = grp.geometry
    assert (geo["block48"], geo["convert16"], geo["frames"], geo["skip_head"], geo["return_length"]) == \
        (blk, 13920, 87, 50, 37)
    rngs = _rngs(g)
    opts = grp.opts(f0_up_key=float(g["f0_up_key"]), protect=float(g["protect"]), index_rate=0.0)
    same, compared, gated = 0, 0, 0
    for h in range(H):
        ez, es = hop_noise(rngs, *_sizes(grp))
        out, vol = grp.process(x[:, h * blk:(h + 1) * blk], opts, eps_z=ez, eps_src=es)
        torch.cuda.synchronize()
        out, vol, offs = out.cpu().numpy(), vol.cpu().numpy(), grp.offs.cpu().numpy()
        assert np.isfinite(out).all()
        for s in range(S):
            ref = g["out16"][s, h].astype(np.float32)
            rv = float(g["vol"][s, h])
            assert abs(float(vol[s]) - rv) <= 1e-5 * max(rv, 1e-12), (h, s, vol[s], rv)
            if rv == 0.0:  # gated hop: zeros through SOLA -> offset 0, output = the crossfade tail
                gated += 1
                assert offs[s] == 0 == int(g["sola_offset"][s, h])
                np.testing.assert_allclose(out[s], ref, atol=2e-3 * max(1e-3, float(np.abs(ref).max())))
                continue
            if bool(g["unsure"][s, h]):
                continue
            if h == 0:  # first hop: the SOLA buffer is zeros, every offset ties at 0
                assert offs[s] == int(g["sola_offset"][s, h]) == 0
            compared += 1
            same += int(offs[s] == int(g["sola_offset"][s, h]))
            if offs[s] == int(g["sola_offset"][s, h]):
                peak = float(np.abs(ref).max())
                assert float(np.abs(out[s] - ref).max()) <= 2e-3 * peak, (h, s, float(np.abs(out[s] - ref).max()), peak)
            assert spectrogram_correlation(out[s], ref) >= 0.999, (h, s)
    engine.check_device_status()
    grp.close()
    assert gated >= 1 and compared >= 0.75 * (S * H - gated)
    assert same >= 0.95 * compared, (same, compared)


def test_voice_changer_fcpe_equals_stream_0_of_a_group(engine, fx):
    """One-stream VoiceChanger(..., f0_method="fcpe").on_request against stream 0 of a 4-stream group fed the same
    blocks and noise: the same bars (the batch may pick another GEMM split, so not bit equality), equal SOLA offsets."""
    from oracle.metrics import spectrogram_correlation
    from rvcx.realtime import StreamGroup, VoiceChanger

    g, x = fx["g"], fx["x"]
    S, H, blk = int(g["n_streams"]), int(g["hops"]), int(g["block"])
    thr = float(g["threshold"])
    sids = [int(v) for v in g["sids"]]
    grp = StreamGroup(engine, S, sid=sids, f0_method="fcpe", fcpe_threshold=thr, **GEOM)
    vc = VoiceChanger(96, 0.1, 0.5, engine=engine, silent_threshold=-90, sid=sids[0], f0_method="fcpe",
                      fcpe_threshold=thr)
    assert vc.group.f0_method == "fcpe" and vc.block_frame == blk
    rngs = _rngs(g)
    kw = dict(f0_up_key=float(g["f0_up_key"]), protect=float(g["protect"]), index_rate=0.0)
    for h in range(H):
        ez, es = hop_noise(rngs, *_sizes(grp))
        out, vol = grp.process(x[:, h * blk:(h + 1) * blk], grp.opts(**kw), eps_z=ez, eps_src=es)
        torch.cuda.synchronize()
        ref, rv, roff = out[0].cpu().numpy(), float(vol[0].item()), int(grp.offs[0].item())
        vc.process_audio = functools.partial(VoiceChanger.process_audio, vc, eps_z=ez[:1], eps_src=es[:1])
        res, v1, lat = vc.on_request(x[0, h * blk:(h + 1) * blk].copy(), **kw)
        assert res.shape == (blk,) and res.dtype == np.float32 and np.isfinite(res).all() and len(lat) == 3
        assert rv > 0 and abs(v1 - rv) <= 1e-5 * rv
        assert int(vc.group.offs[0].item()) == roff, (h, int(vc.group.offs[0].item()), roff)
        peak = float(np.abs(ref).max())
        assert float(np.abs(res - ref).max()) <= 2e-3 * peak, (h, float(np.abs(res - ref).max()), peak)
        assert spectrogram_correlation(res, ref) >= 0.999, h
    vc.close()
    grp.close()


def test_fcpe_streams_need_fcpe_not_rmvpe(engine, fx, synth_w, hubert_w):
    """An Engine with the synthesizer, HuBERT and FCPE but no RMVPE runs "fcpe" streams and refuses "rmvpe" with the
    state error; an Engine without FCPE refuses "fcpe" naming load_fcpe; an unknown name is refused by name."""
    from rvcx import _lib
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup, VoiceChanger

    g, x = fx["g"], fx["x"]
    blk = int(g["block"])
    e = Engine(0)
    try:
        e.load_synth(synth_w, SYNTH_48K_V2)
        e.load_hubert(hubert_w)
        with pytest.raises(ValueError, match="load_fcpe"):
            StreamGroup(e, 2, f0_method="fcpe", **GEOM)
        with pytest.raises(ValueError, match="load_fcpe"):
            VoiceChanger(96, 0.1, 0.5, engine=e, silent_threshold=-90, f0_method="fcpe")
        with pytest.raises(ValueError, match="rmvpe.*fcpe"):
            StreamGroup(e, 2, f0_method="crepe", **GEOM)
        e.load_fcpe(*_fcpe_weights(g))
        with pytest.raises(_lib.RvcxError, match="RMVPE") as err:
            StreamGroup(e, 2, f0_method="rmvpe", **GEOM)
        assert err.value.code == -5  # RVCX_E_STATE
        grp = StreamGroup(e, 2, f0_method="fcpe", fcpe_threshold=float(g["threshold"]), **GEOM)
        out, vol = grp.process(x[:2, :blk], grp.opts(index_rate=0.0), seed=1)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and float(out.abs().max()) > 0 and (vol > 0).all()
        e.check_device_status()
        grp.close()
    finally:
        e.close()


def test_zero_initialised_desc_still_runs_rmvpe(engine, fx):
    """A rvcx_rt_desc whose two new trailing fields are zero behaves as before they existed: RMVPE. Its hop is bit
    equal to a default ("rmvpe") group's and differs from an "fcpe" group's."""
    from rvcx import _lib
    from rvcx.realtime import StreamGroup

    g, x = fx["g"], fx["x"]
    blk = int(g["block"])
    groups = {m: StreamGroup(engine, 2, f0_method=m, fcpe_threshold=float(g["threshold"]), **GEOM)
              for m in ("rmvpe", "fcpe")}
    raw = StreamGroup(engine, 2, **GEOM)
    d = _lib.RtDesc()  # ctypes zero-initialises
    assert d.f0_method == 0 and d.fcpe_threshold == 0.0
    d.n_streams, d.read_chunk_size = 2, GEOM["read_chunk_size"]
    d.cross_fade_overlap_size, d.extra_convert_size = GEOM["cross_fade_overlap_size"], GEOM["extra_convert_size"]
    d.silent_threshold = GEOM["silent_threshold"]
    h = ctypes.c_void_p()
    engine._check(engine.lib.rvcx_rt_create(engine.ctx, ctypes.byref(d), ctypes.byref(h)), "rt_create")
    raw.close()
    raw.handle = h
    ez, es = hop_noise(_rngs(g)[:2], *_sizes(raw))
    outs = {}
    for name, grp in (("rmvpe", groups["rmvpe"]), ("fcpe", groups["fcpe"]), ("raw", raw)):
        out, _ = grp.process(x[:2, :blk], grp.opts(index_rate=0.0, protect=0.33), eps_z=ez, eps_src=es)
        torch.cuda.synchronize()
        outs[name] = out.clone()
        grp.close()
    assert torch.isfinite(outs["raw"]).all()
    assert torch.equal(outs["raw"], outs["rmvpe"])
    assert not torch.equal(outs["raw"], outs["fcpe"])
    dd = _lib.RtDesc()
    engine.lib.rvcx_rt_default_desc(ctypes.byref(dd))
    assert dd.f0_method == 0 and abs(dd.fcpe_threshold - 0.006) < 1e-9
    dd.f0_method = 2
    with pytest.raises(_lib.RvcxError, match="f0_method"):
        engine._check(engine.lib.rvcx_rt_create(engine.ctx, ctypes.byref(dd), ctypes.byref(ctypes.c_void_p())),
                      "rt_create")
