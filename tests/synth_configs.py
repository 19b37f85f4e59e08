"""The synthesizer configurations beside SYNTH_48K_V2 that the suite runs (test helper, no GPU needed).

    name     upsample_rates   kernels         sr     phone width   source
    v2_40k   10,10,2,2        16,16,4,4       40000  768           the reference's rvc/configs/40000.json
    v2_32k   10,8,2,2         20,16,4,4       32000  768           the reference's rvc/configs/32000.json
    v1_48k   10,6,2,2,2       16,16,4,4,4     48000  256           the list v1 48 kHz checkpoints carry in cpt["config"]
    v1_32k   10,4,2,2,2       16,16,4,4,4     32000  256           the list v1 32 kHz checkpoints carry

What each one reaches that SYNTH_48K_V2 (12,10,2,2 / 24,20,4,4: k = 2u at every stage, polyphase taps 3, pad 1, every
slot of the packed ConvTranspose weight live) does not: v2_40k k = 16, u = 10, p = 3 (of the three packed taps, phases
0..2 and 7..9 have two live, phases 3..6 one, the other slots are zero-filled); v2_32k noise strides 32 / 4 / 2 and upp 320; the v1 lists five stages ending at 16
channels (the generic conv_post, ResBlocks at N = 16) and 256-dim phone features; v1_32k u = 4, k = 16: taps 5, pad 2.
Weights are seeded (rvcx.synthetic.synth_state), nothing is read from a file.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from rmvpe_parity import check_rmvpe, margins, rel_err, trim_normalize
from rvcx.config import SYNTH_48K_V2

CONFIGS = {
    "v2_40k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 10, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                                  sr=40000),
    "v2_32k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 8, 2, 2), upsample_kernel_sizes=(20, 16, 4, 4),
                                  sr=32000),
    "v1_48k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 6, 2, 2, 2),
                                  upsample_kernel_sizes=(16, 16, 4, 4, 4), sr=48000, text_enc_hidden_dim=256),
    "v1_32k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 4, 2, 2, 2),
                                  upsample_kernel_sizes=(16, 16, 4, 4, 4), sr=32000, text_enc_hidden_dim=256),
}
NAMES = tuple(CONFIGS)
SEED_W = 7  # synthetic.synth_state seed of every configuration's weights

_W = {}


def version_of(cfg) -> str:
    """The HuBERT output the configuration's TextEncoder takes: "v1" (final_proj, 256) or "v2" (768)."""
    return "v1" if cfg.text_enc_hidden_dim == 256 else "v2"


def weights_for(name):
    """normalize_state(synthetic.synth_state(SEED_W, cfg)), built once per configuration and never modified."""
    if name not in _W:
        from rvcx import synthetic
        from rvcx.weights import normalize_state

        _W[name] = normalize_state(synthetic.synth_state(SEED_W, CONFIGS[name]))
    return _W[name]


def margin_frames(cfg) -> int:
    """rvcx_dec_margin_frames(cfg): host only, no context and no GPU."""
    import ctypes

    from rvcx import _lib
    from rvcx.engine import Engine

    d = Engine._synth_desc(cfg)
    m = ctypes.c_int32(0)
    rc = _lib.load().rvcx_dec_margin_frames(ctypes.byref(d), ctypes.byref(m))
    assert rc == 0, rc
    return m.value


def pipeline_vs_oracle(cfg_engine, clip, hubert_w, rmvpe_w):
    """The decomposition and the bars of test_gpu_sizes.py rows 1-2 (and test_gpu_c2_parity.py's pipeline == staged):
    output shape; the salience-aware f0 check; voice_conversion fed the oracle's pitch within 1e-4 of the peak after
    the configuration's trim; the pipeline within 1e-6 of the staged path; spectrogram correlation >= 0.999. Shared
    with tests/test_gpu_refinegan.py (the oracle draws the decoder's own noise layout); returns (audio, eps_z, eps_src,
    the pipeline's output) for what a caller checks on top."""
    from oracle.metrics import spectrogram_correlation
    from oracle.pipeline import OraclePipeline
    from rvcx.config import HUBERT_BASE, RMVPE_CFG
    from pipeline_ref import NoiseRecorder

    name, cfg, w, eng = cfg_engine
    audio, sal_gap = clip
    noise = NoiseRecorder(70)
    orc = OraclePipeline(cfg.sr, synth_w=w, synth_cfg=cfg, hubert_w=hubert_w, hubert_cfg=HUBERT_BASE, rmvpe_w=rmvpe_w,
                         rmvpe_cfg=RMVPE_CFG, noise_fn=noise)
    ref = orc.pipeline(0, audio.copy(), protect=0.33, version=version_of(cfg))
    ez, es = noise.cat()
    sal = margins(orc.last["hidden"])
    sal["sal_fp32_noise"] = sal_gap
    f0_ref, pitch_ref = orc.last["f0_raw"], np.asarray(orc.last["pitch"], np.int64)

    eng.set_pipeline_highpass()
    out, f0p = eng.pipeline(audio, sid=0, semitones=0, protect=0.33, t_pad=16000, t_pad_tgt=cfg.sr, eps_z=ez,
                            eps_src=es, want_f0=True)
    _, p32 = eng.highpass_pad(audio, 16000)
    f0d, hid = eng.rmvpe(p32, want_hidden=True)
    eng.check_device_status()
    out, f0p, f0d, hid = (v.cpu().numpy() for v in (out, f0p, f0d, hid))
    assert out.shape == ref.shape
    np.testing.assert_array_equal(f0p, f0d)
    assert rel_err(hid, np.asarray(orc.last["hidden"], np.float32)) <= 1e-3
    r = check_rmvpe(f0d, hid, sal, f0_ref)
    c = spectrogram_correlation(out, ref)
    P = p32.shape[0] // 160
    vc = trim_normalize(eng.voice_conversion(p32, pitch_ref[:P], f0_ref[:P].astype(np.float32), 0, 0.33, eps_z=ez,
                                             eps_src=es).cpu().numpy(), cfg.sr)
    e_ref = rel_err(vc, ref)
    coarse, pitchf, _ = eng.f0_post(f0d, 0.0)
    vcd = trim_normalize(eng.voice_conversion(p32, coarse[:P], pitchf[:P], 0, 0.33, eps_z=ez,
                                              eps_src=es).cpu().numpy(), cfg.sr)
    cons = rel_err(out, vcd)
    eng.check_device_status()
    print(f"\n{name} pipeline: salience err {r['err']:.2e} (bound {3 * sal_gap:.2e}), {r['n_near']} near-tied, flips "
          f"{list(r['flips'])[:8]}, spec corr {c:.6f}, vc on oracle pitch {e_ref:.2e}, pipeline vs staged {cons:.1e}")
    assert e_ref <= 1e-4, e_ref
    assert cons <= 1e-6, cons
    assert c >= 0.999, c
    return audio, ez, es, out


def stream_group_vs_oracle(cfg_engine, hubert_w, rmvpe_w, hops=3, src_noise=None):
    """test_gpu_stream.test_stream_group_matches_oracle with a 40 kHz model: the hop's output goes through the second
    sinc resample tgt_sr -> 48000. That test's bars (geometry equal, vol rel <= 1e-5, SOLA offsets equal on >= 75 % of
    hops, per-hop spectrogram corr > 0.99) and, on hops whose offset equals the oracle's, max |diff| <= 2e-3 of the
    hop's peak (test_gpu_stream_ref.py). src_noise(rng, B, T) -> (the group's eps_src, [row b's own B = 1 block]) for a
    decoder whose source noise is not [B][T upp] (tests/test_gpu_refinegan.py)."""
    from oracle.metrics import spectrogram_correlation
    from oracle.realtime import OracleVoiceChanger
    from rvcx import synthetic
    from rvcx.config import HUBERT_BASE, RMVPE_CFG
    from rvcx.realtime import StreamGroup

    name, cfg, w, eng = cfg_engine
    B, protect = 2, 0.33
    orc = [OracleVoiceChanger(w, cfg, hubert_w, HUBERT_BASE, rmvpe_w, RMVPE_CFG, read_chunk_size=96,
                              silent_threshold=-90.0, sid=b) for b in range(B)]
    grp = StreamGroup(eng, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=[0, 1])
    try:
        g, o0 = grp.geometry, orc[0]
        assert (g["block48"], g["block16"], g["convert16"], g["frames"], g["skip_head"], g["return_length"],
                g["crossfade48"], g["sola_search48"]) == \
            (o0.block_frame, o0.audio_buffer.numel() - int(o0.crossfade_frame / 48000 * 16000),
             o0.convert_buffer.numel(), o0.convert_feature_size_16k, o0.skip_head, o0.return_length,
             o0.crossfade_frame, o0.sola_search_frame)
        block, T, I, upp = g["block48"], g["frames"], cfg.inter_channels, cfg.upp
        audio = np.stack([synthetic.speech_like(block * hops, seed=60 + b, sr=48000).astype(np.float32)
                          for b in range(B)])
        rng = np.random.default_rng(7)
        same_off, n_off = 0, 0
        for h in range(hops):
            x = audio[:, h * block:(h + 1) * block]
            ez = rng.standard_normal((B, I, T)).astype(np.float32)
            if src_noise is None:
                es = rng.standard_normal((B, T * upp)).astype(np.float32)
                es_rows = [es[b:b + 1] for b in range(B)]
            else:
                es, es_rows = src_noise(rng, B, T)
            out, vol = grp.process(x, grp.opts(protect=protect), eps_z=ez, eps_src=es)
            torch.cuda.synchronize()
            eng.check_device_status()
            out, vol, offs = out.cpu().numpy(), vol.cpu().numpy(), grp.offs.cpu().numpy()
            for b in range(B):
                it = iter([torch.from_numpy(ez[b:b + 1]), torch.from_numpy(es_rows[b])])
                orc[b].noise_fn = lambda shape, which, it=it: next(it)
                ref, rvol = orc[b].on_request(x[b].copy(), protect=protect)
                assert ref.shape == out[b].shape and np.any(ref)
                assert abs(vol[b] - rvol) <= 1e-5 * max(rvol, 1e-12), (h, b, vol[b], rvol)
                n_off += 1
                same = int(offs[b]) == orc[b].last["sola_offset"]
                same_off += int(same)
                corr = spectrogram_correlation(out[b], ref)
                peak = float(np.abs(ref).max())
                d = float(np.abs(out[b] - ref).max())
                print(f"\n{name} stream hop {h} row {b}: offset {int(offs[b])} / {orc[b].last['sola_offset']}, spec corr "
                      f"{corr:.6f}, max |diff| {d / peak:.2e} of the peak")
                assert corr > 0.99, (h, b, corr)
                if same:
                    assert d <= 2e-3 * peak, (h, b, d, peak)
        assert same_off >= 0.75 * n_off, (same_off, n_off)
    finally:
        grp.close()
