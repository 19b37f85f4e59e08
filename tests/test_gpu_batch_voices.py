"""A voice per batch row (rvcx_pipeline_batch_voices, Engine.pipeline_batch_v(voices=), RVCX.convert_many(voices=)): the
high-pass, the ragged HuBERT and the pitch network run once over all rows, retrieval and Synthesizer.infer once per
voice on its row range.

Rows ragged_rows.PIPE_NS with SHORT_PAD, voices [A, A, B, B] (synthetic.synth_state(2 / 3) at SYNTH_48K_V2, each with
its own small IVF index, index_rate 0.5):
* every row against pipeline_ex under its own voice with its slice of the injected noise at compare_row's bars
  (correlation > 0.999, difference < 5e-3 of the peak); under f0_method 0 the row's f0 equals the single run's bit for
  bit, since the pitch pass does not depend on the voice;
* once more inside an arena of the maximum of workspace_bytes(B, n_max, opts) over the voices in use, without
  RVCX_E_OOM and with the same bits;
* convert_many(audios, voices=[B, A, B, A]) returns in input order, each output against the single-utterance conversion
  under that voice at the bars of test_convert_many_matches_convert_per_clip."""
import numpy as np
import pytest

from ragged_rows import PIPE_NS, PIPE_SIDS, SHORT_PAD, clip, compare_row, noise_for
from voice_bank_common import SEED_A, SEED_B, assert_separated, bank_engine, weights

pytestmark = pytest.mark.gpu


def test_mixed_batch_rows_match_single_runs(hubert_w, rmvpe_w):
    eng, ids = bank_engine(hubert_w, rmvpe_w, [SEED_A, SEED_B])
    try:
        eng.set_pipeline_highpass()
        A, B = ids[SEED_A], ids[SEED_B]
        voices = [A, A, B, B]
        rows = [clip(n, 90 + b) for b, n in enumerate(PIPE_NS)]
        kw = dict(pitch=2.0, index_rate=0.5, f0_method=0, **SHORT_PAD)
        opts = eng.pipeline_opts(**kw)
        upp = eng.upp
        Ts, ez, es = noise_for(eng, rows, opts, 61)
        ys, f0s = eng.pipeline_batch_v(rows, opts, sids=PIPE_SIDS, eps_z=ez, eps_src=es, want_f0=True, voices=voices)
        ys, f0s = [eng.host(y) for y in ys], [eng.host(f) for f in f0s]
        assert eng.voice == 0

        def single(b, voice):
            eng.select_voice(voice)
            y1, f1 = eng.pipeline_ex(rows[b], eng.pipeline_opts(sid=PIPE_SIDS[b], **kw),
                                     eps_z=np.ascontiguousarray(ez[b, :, :Ts[b]]).reshape(-1),
                                     eps_src=es[b, :Ts[b] * upp], want_f0=True)
            eng.select_voice(0)
            return eng.host(y1), eng.host(f1)

        assert_separated("row 2 under A / B", single(2, A)[0], single(2, B)[0])
        failed = []
        for b, v in enumerate(voices):
            y1, f1 = single(b, v)
            assert ys[b].shape == y1.shape == (Ts[b] * upp - 2 * int(opts.t_pad_tgt),), (b, ys[b].shape, y1.shape)
            failed += compare_row(f"row {b} n={len(rows[b])} voice {v}", ys[b], y1, f0s[b], f1)
            np.testing.assert_array_equal(f0s[b], f1, err_msg=f"row {b}: f0 is the single run's under f0_method 0")
        assert not failed, "; ".join(failed)
        # voices = None is rvcx_pipeline_batch_v itself, and a batch of one voice given as such equals it bit for bit
        plain = eng.pipeline_batch_v(rows, opts, sids=PIPE_SIDS, eps_z=ez, eps_src=es)
        as_a = eng.pipeline_batch_v(rows, opts, sids=PIPE_SIDS, eps_z=ez, eps_src=es, voices=A)
        for p, q in zip(plain, as_a):
            np.testing.assert_array_equal(eng.host(p), eng.host(q))
        # the stated arena holds the call
        need = 0
        for v in sorted(set(voices)):
            eng.select_voice(v)
            need = max(need, eng.workspace_bytes(max(PIPE_NS), B=len(rows), opts=opts))
        eng.select_voice(0)
        arena = eng.torch.empty((need,), dtype=eng.torch.uint8, device=eng.device)
        eng.set_workspace(arena)
        try:
            again = eng.pipeline_batch_v(rows, opts, sids=PIPE_SIDS, eps_z=ez, eps_src=es, voices=voices)
            again = [eng.host(y) for y in again]
            print(f"\narena {need} B, carved {eng.workspace_info()[2]} B")
        finally:
            eng.set_workspace(None)
        for b in range(len(rows)):
            np.testing.assert_array_equal(again[b], ys[b], err_msg=f"row {b} inside the arena")
        eng.check_device_status()
    finally:
        eng.close()


def test_convert_many_with_a_voice_per_utterance(hubert_w, rmvpe_w):
    from oracle.metrics import spectrogram_correlation
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer import RVCX, Config

    ns = [9600, 8000, 12000, 10400]
    clips = [clip(n, 50 + i) for i, n in enumerate(ns)]
    cfg = Config()
    cfg.x_pad = 0.3  # the clips are shorter than the default 1 s pad, which the reflect padding refuses
    rvc = RVCX(config=cfg, synth_state=weights(SEED_A), synth_cfg=SYNTH_48K_V2, hubert_state=hubert_w,
               rmvpe_state=rmvpe_w)
    try:
        a = rvc.default_voice
        b = rvc.add_voice(synth_state=weights(SEED_B), synth_cfg=SYNTH_48K_V2, name="b")
        assert rvc.voices == [a, "b"] and rvc.engine.voice == 0
        with pytest.raises(KeyError):
            rvc.convert(clips[0], voice="nobody")
        with pytest.raises(ValueError):
            rvc.add_voice(synth_state=weights(SEED_B), synth_cfg=SYNTH_48K_V2, name="b")
        upp = rvc.engine.upp
        names = [b, a, b, a]

        def noise_fn(i, T):
            r = np.random.default_rng(1000 + i)
            return r.standard_normal((192, T)).astype(np.float32), r.standard_normal(T * upp).astype(np.float32)

        outs = rvc.convert_many(clips, pitch=2, protect=0.33, sid=3, batch=4, max_pad=0.5, noise_fn=noise_fn,
                                voices=names)
        assert len(outs) == len(clips) and rvc.engine.voice == 0 and rvc.tgt_sr == 48000

        def single(i, name):
            ez, es = noise_fn(i, (outs[i].shape[0] + 2 * rvc.pipeline.t_pad_tgt) // upp)
            rvc.engine.select_voice(rvc.voices.index(name))  # ids follow the order the voices were added in
            y = rvc.pipeline.pipeline(rvc.hubert_model, rvc.net_g, 3, clips[i], 2, "rmvpe", None, 0.0, True, 1.0, "v2",
                                      0.33, eps_z=ez.reshape(-1), eps_src=es)
            rvc.engine.select_voice(0)
            return y

        assert_separated("clip 0 under a / b", single(0, a), single(0, b))
        for i, name in enumerate(names):
            y1 = single(i, name)
            assert outs[i].shape == y1.shape and outs[i].dtype == np.float32
            corr = spectrogram_correlation(outs[i], y1)
            diff = float(np.abs(outs[i] - y1).max()) / max(float(np.abs(y1).max()), 1e-6)
            print(f"\nclip {i} n={ns[i]} voice {name}: corr {corr:.6f} max diff / peak {diff:.3e}")
            assert corr > 0.999 and diff < 5e-3
        # convert(voice=) runs on that voice and leaves the default as it was
        y_b = rvc.convert(clips[1], pitch=2, protect=0.33, sid=3, seed=5, voice=b)
        y_a = rvc.convert(clips[1], pitch=2, protect=0.33, sid=3, seed=5)
        assert y_b.shape == y_a.shape and rvc.engine.voice == 0
        assert_separated("convert(voice=)", y_a, y_b)
        np.testing.assert_array_equal(y_a, rvc.convert(clips[1], pitch=2, protect=0.33, sid=3, seed=5, voice=a))
        assert rvc.output_sr(0, b) == 48000 and rvc.output_sr(16000, b) == 16000
    finally:
        rvc.close()
