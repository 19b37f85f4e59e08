"""HuBERT over a batch of rows of different lengths (rvcx_hubert_batch_v), against the oracle in float64 and against
the single-row path.

The batch: n = 40000, 400, 21000, 20700, 16000 samples -> L = 124, 1, 65, 64, 49 frames: the longest row first, a row
of one frame, one row on each side of the positional conv's half-width 64 (its taps reach 64 frames past a row's end,
where a ragged batch holds another row's pad frames instead of the zero padding), and a shorter row last. The same
rows reversed put the longest last."""
import numpy as np
import pytest

import parity_anchor as pa
import ragged_rows
from parity_anchor import K, anchor, check
from ragged_rows import SHORT_PAD, clip, noise_for, speech

pytestmark = pytest.mark.gpu

NS = (40000, 400, 21000, 20700, 16000)
LS = (124, 1, 65, 64, 49)


@pytest.fixture(scope="module")
def rows(hubert_w):
    """Per row: the audio, the oracle's float64 features and the fp32-vs-fp64 gap (computed once for all tests)."""
    out = []
    for b, n in enumerate(NS):
        audio = speech(n, seed=60 + b)
        ref, gap = anchor(pa.hubert_fn(hubert_w, audio[None]))["out"]
        assert ref.shape == (1, LS[b], 768)
        out.append((audio, ref[0], gap))
    return out


@pytest.fixture(scope="module")
def single(engine, rows):
    """engine.hubert on every row alone."""
    return [engine.host(engine.hubert(a)) for a, _, _ in rows]


@pytest.mark.parametrize("order", ["longest_first", "longest_last"])
def test_ragged_hubert_vs_fp64_and_single(engine, rows, single, order):
    idx = list(range(len(NS))) if order == "longest_first" else list(reversed(range(len(NS))))
    # longest_last also leaves room between the rows' blocks (ld_rows > the longest row's frames: the strided copy)
    ld = None if order == "longest_first" else max(LS) + 3
    feats = engine.hubert_batch_v([rows[i][0] for i in idx], ld_rows=ld)
    assert len(feats) == len(idx)
    failed = []
    for f, i in zip(feats, idx):
        _, ref, gap = rows[i]
        f = engine.host(f)
        assert f.shape == (LS[i], 768), (NS[i], f.shape)
        try:
            check(f"hubert_batch_v {order} row n={NS[i]} vs fp64", f, ref, gap, K)
            # two honest fp32 evaluations each sit at most one gap from float64
            check(f"hubert_batch_v {order} row n={NS[i]} vs single", f, single[i], gap, 2)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def test_equal_lengths_take_the_equal_length_path(engine):
    """All-equal lengths and B = 1 are accepted and give hubert_batch's / hubert's bits."""
    audio = np.stack([speech(5000, seed=70 + b) for b in range(3)])
    eq = engine.host(engine.hubert_batch(audio))
    got = engine.hubert_batch_v(list(audio))
    assert all(np.array_equal(engine.host(g), eq[b]) for b, g in enumerate(got))
    one = engine.hubert_batch_v([audio[1]])
    assert np.array_equal(engine.host(one[0]), engine.host(engine.hubert(audio[1])))


def test_stale_scratch_does_not_reach_the_output(engine, rows):
    """A caller may write its arena between calls: with the work buffers full of NaN bit patterns or of zeros before
    the call, the ragged pass gives the same bits, all finite (a pad frame read before it was written would show)."""
    t = engine.torch
    audios = [rows[i][0] for i in (2, 0, 4)]
    arena = t.empty(256 << 20, dtype=t.uint8, device=engine.device)  # ~100 MB of conv activations for these rows
    engine.set_workspace(arena)
    try:
        outs = []
        for fill in (0xFF, 0x00):
            arena.fill_(fill)
            outs.append([engine.host(f) for f in engine.hubert_batch_v(audios)])
    finally:
        engine.set_workspace(None)
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_refusals(engine):
    from rvcx._lib import RvcxError

    with pytest.raises(RvcxError) as e:  # a row shorter than one frame, as rvcx_hubert refuses it
        engine.hubert_batch_v([speech(5000, 1), speech(399, 2)])
    assert e.value.code == -2
    with pytest.raises(RvcxError) as e:  # blocks too small for the longest row's frames
        engine.hubert_batch_v([speech(5000, 1), speech(9000, 2)], ld_rows=20)
    assert e.value.code == -6


# ----------------------------------------------------------------- the ragged pipeline (rvcx_pipeline_batch_v)
def check_rows_vs_single(engine, audios, sids, seed, **kw):
    """Every row of the ragged pass against pipeline_ex on that utterance alone with its slice of the noise: equal
    shape and n_out, spectrogram correlation > 0.999, max difference < 5e-3 of the peak
    (test_pipeline_batch_matches_single's bars), and the same adjusted f0: bit for bit for a row whose length no other
    row has (it runs the single-row RMVPE forward). Rows of equal length share one batched RMVPE pass, whose kernels
    sum in another order than the single-row ones (as rvcx_rmvpe_batch against rvcx_rmvpe): the same voicing decisions
    and f0 within 0.1 cent. That is the roundoff of the decode, not a bar fitted to the result: f0 is 10 * 2^(c / 1200)
    with c the salience-weighted mean of nine 20-cent bins, so two fp32 evaluations of the salience, each within the
    5e-5 (absolute) fp32-vs-float64 gap of DESIGN.md section 5 on weights that sum to at least the 0.03 threshold, move
    c by at most 2 * 5e-5 * (sum of |bin - mean| <= 400 cents) / 0.03 = 1.3 cents in the worst case and by about 0.01
    cent at typical weight sums near 1; 0.1 cent lies between and is 500 times tighter than the 50 cents of the oracle
    tests."""
    from oracle.metrics import spectrogram_correlation

    def judge(b, name, y, y1, f0, f1):
        failed = []
        corr = spectrogram_correlation(y, y1)
        diff = float(np.abs(y - y1).max()) / max(float(np.abs(y1).max()), 1e-6)
        df0 = float(np.abs(f0 - f1).max()) if f0.shape == f1.shape else float("inf")
        print(f"\n{name}: corr {corr:.6f} max diff / peak {diff:.3e} max |f0 diff| {df0:.3e}")
        if not (corr > 0.999 and diff < 5e-3):
            failed.append(f"{name}: corr {corr:.6f} diff {diff:.3e}")
        if sum(len(x) == len(audios[b]) for x in audios) == 1:
            if not np.array_equal(f0, f1):
                failed.append(f"{name}: f0 differs from the single run's by up to {df0:.3e}")
        else:
            voiced = f1 > 0
            cents = float(np.abs(1200.0 * np.log2(f0[voiced] / f1[voiced])).max()) if voiced.any() else 0.0
            print(f"{name} (batched RMVPE subgroup): max f0 difference {cents:.4f} cent")
            if not (np.array_equal(f0 > 0, voiced) and cents <= 0.1):
                failed.append(f"{name}: f0 differs from the single run's by {cents:.4f} cent or in voicing")
        return failed

    ragged_rows.check_rows_vs_single(engine, audios, sids, seed, {}, {}, judge, pitch=2.0, protect=0.33, **kw)


def test_ragged_pipeline_matches_single(engine):
    """n = 24000, 40000, 8000, 24000 with sids 0, 3, 7, 0: the two rows of equal length share one batched RMVPE pass."""
    ns = [24000, 40000, 8000, 24000]
    check_rows_vs_single(engine, [clip(n, 90 + b) for b, n in enumerate(ns)], [0, 3, 7, 0], seed=3, **SHORT_PAD)


def test_ragged_pipeline_volume_envelope(engine):
    check_rows_vs_single(engine, [clip(n, 95 + b) for b, n in enumerate([18000, 30000, 22000])], [0, 1, 2], seed=4,
                         volume_envelope=0.5)


def test_ragged_pipeline_with_index(engine):
    """index_rate = 0.5 with an index built on device (as tests/test_gpu_index_build.py builds one): retrieval runs over
    all B * L_max rows, pad rows included, and only the valid rows' results are used."""
    from rvcx import synthetic

    feats = engine.host(engine.hubert(synthetic.speech_like(16000 * 4, seed=31).astype(np.float32)))
    engine.index_build(feats, 6, niter=8, seed=1)
    try:
        check_rows_vs_single(engine, [clip(n, 97 + b) for b, n in enumerate([18000, 26000, 20000])], [0, 0, 5], seed=5,
                             index_rate=0.5)
    finally:
        engine.index_unload()


def test_ragged_pipeline_vs_reference_fixture(engine):
    """The reference's own Pipeline.pipeline output (tests/golden/pipeline_2p5s.npz) as the middle row of a three-row
    ragged batch, with its recorded noise: test_pipeline_batch_vs_reference_and_oracle's bars."""
    from conftest import golden
    from oracle.metrics import spectrogram_correlation

    engine.set_pipeline_highpass()
    g = golden("pipeline_2p5s.npz")
    n = g["audio"].shape[0]
    audios = [clip(24000, 81), g["audio"], clip(n + 8000, 82)]
    opts = engine.pipeline_opts(protect=0.33)
    Ts, ez, es = noise_for(engine, audios, opts, 6)
    ez[1, :, :Ts[1]] = g["eps_z"].reshape(192, Ts[1])
    es[1, :Ts[1] * engine.upp] = g["eps_src"].reshape(-1)
    y = engine.host(engine.pipeline_batch_v(audios, opts, sids=0, eps_z=ez, eps_src=es)[1])
    assert y.shape == g["out"].shape
    corr = spectrogram_correlation(y, g["out"])
    rel = float(np.abs(y.astype(np.float64) - g["out"]).max() / (np.abs(g["out"]).max() + 1e-12))
    print(f"\nfixture row: corr {corr:.6f} rel {rel:.3e}")
    assert corr >= 0.999 and rel <= 2e-3


def test_ragged_pipeline_stale_scratch(engine):
    """An arena of workspace_bytes(n_max, B) holds the ragged pass (no RVCX_E_OOM), and its contents before the call
    (NaN bit patterns or zeros) do not reach the output: bit-identical, finite rows."""
    t = engine.torch
    engine.set_pipeline_highpass()
    ns = [24000, 40000, 8000, 24000]
    audios = [clip(n, 90 + b) for b, n in enumerate(ns)]
    opts = engine.pipeline_opts(pitch=2.0, protect=0.33, **SHORT_PAD)
    arena = t.empty(engine.workspace_bytes(max(ns), len(ns), opts), dtype=t.uint8, device=engine.device)
    engine.set_workspace(arena)
    try:
        outs = []
        for fill in (0xFF, 0x00):
            arena.fill_(fill)
            outs.append([engine.host(y) for y in engine.pipeline_batch_v(audios, opts, sids=[0, 3, 7, 0], seed=11)])
    finally:
        engine.set_workspace(None)
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_ragged_pipeline_refusals_and_equal_lengths(engine):
    from rvcx._lib import RvcxError

    engine.set_pipeline_highpass()
    a, b = clip(24000, 1), clip(30000, 2)
    # the generator's receptive field is 10 frames of 480 samples: a smaller t_pad_tgt cannot hide a shorter row's tail
    small = engine.pipeline_opts(t_pad_tgt=9 * engine.upp)
    with pytest.raises(RvcxError) as e:
        engine.pipeline_batch_v([a, b], small)
    assert e.value.code == -1 and "receptive field" in str(e.value)
    assert len(engine.pipeline_batch_v([a, a.copy()], small, seed=1)) == 2  # equal lengths: nothing to hide
    with pytest.raises(RvcxError) as e:  # a row above t_max, as rvcx_pipeline_batch refuses it
        engine.pipeline_batch_v([a, b], engine.pipeline_opts(t_max=30000))
    assert e.value.code == -1 and "t_max" in str(e.value)
    # B = 1 and all-equal lengths are accepted; equal lengths give rvcx_pipeline_batch's bits
    opts = engine.pipeline_opts(pitch=2.0)
    one = engine.pipeline_batch_v([a], opts, seed=2)
    assert len(one) == 1 and one[0].shape == (engine.pipeline_frames(len(a), opts) * engine.upp - 2 * 48000,)
    two = np.stack([a, 0.5 * a[::-1]])
    eq = engine.host(engine.pipeline_batch(two, opts, sids=[0, 1], seed=3))
    got = engine.pipeline_batch_v(list(two), opts, sids=[0, 1], seed=3)
    assert all(np.array_equal(engine.host(y), eq[k]) for k, y in enumerate(got))


def test_convert_many_matches_convert_per_clip(synth_w, hubert_w, rmvpe_w):
    """Five seeded clips of 0.5-2.5 s in shuffled order: the results come back in input order, each equal to the
    single-utterance conversion of that clip at the bars above. `convert` draws its noise on the device from its seed,
    and a row of a batch cannot draw what a B = 1 call draws, so both sides get the same injected noise per clip:
    convert_many through noise_fn, the single side through the call `convert` makes (PipelineRVCX.pipeline)."""
    from oracle.metrics import spectrogram_correlation
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer import RVCX, Config

    rng = np.random.default_rng(17)
    ns = [int(n) for n in rng.integers(8000, 40001, size=5)]
    rng.shuffle(ns)
    clips = [clip(n, 50 + i) for i, n in enumerate(ns)]
    cfg = Config()
    cfg.x_pad = 0.3  # the shortest clips are shorter than the default 1 s pad, which the reflect padding refuses
    rvc = RVCX(config=cfg, synth_state=synth_w, synth_cfg=SYNTH_48K_V2, hubert_state=hubert_w, rmvpe_state=rmvpe_w)
    try:
        upp = rvc.engine.upp

        def noise_fn(i, T):
            r = np.random.default_rng(1000 + i)
            return r.standard_normal((192, T)).astype(np.float32), r.standard_normal(T * upp).astype(np.float32)

        outs = rvc.convert_many(clips, pitch=2, protect=0.33, sid=3, batch=4, max_pad=0.5, noise_fn=noise_fn)
        assert len(outs) == len(clips)
        for i, c in enumerate(clips):
            ez, es = noise_fn(i, (outs[i].shape[0] + 2 * rvc.pipeline.t_pad_tgt) // upp)
            y1 = rvc.pipeline.pipeline(rvc.hubert_model, rvc.net_g, 3, c, 2, "rmvpe", None, 0.0, True, 1.0, "v2", 0.33,
                                       eps_z=ez.reshape(-1), eps_src=es)
            assert outs[i].shape == y1.shape and outs[i].dtype == np.float32
            corr = spectrogram_correlation(outs[i], y1)
            diff = float(np.abs(outs[i] - y1).max()) / max(float(np.abs(y1).max()), 1e-6)
            print(f"\nclip {i} n={ns[i]}: corr {corr:.6f} max diff / peak {diff:.3e}")
            assert corr > 0.999 and diff < 5e-3
        # batch = 1 is the per-utterance loop: the same outputs again
        loop = rvc.convert_many(clips, pitch=2, protect=0.33, sid=3, batch=1, noise_fn=noise_fn)
        assert all(a.shape == b.shape for a, b in zip(loop, outs))
    finally:
        rvc.close()
