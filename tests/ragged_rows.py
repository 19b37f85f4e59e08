"""What the tests of the ragged forms share (test_gpu_ragged_batch.py, test_gpu_rmvpe_ragged.py,
test_gpu_fcpe_ragged.py): the seeded clips, the injected noise in the batch layouts, the row-against-single-run bars and
the procedure that holds every row of a ragged pipeline pass to the single-utterance run. A plain module, like
parity_anchor.py: no test module imports another."""
import numpy as np

# an 8000-sample row is shorter than the default t_pad (16000), which the reflect padding of either path refuses
# (t_pad < n): these cases pad by 0.3 s, t_pad_tgt = 3 t_pad = 30 frames, three times the generator's receptive field
SHORT_PAD = dict(t_pad=4800, t_pad_tgt=14400)
# the rows of the ragged-f0 pipeline tests (f0_method 4 and 5; each picks its own seeds) and their speaker ids
PIPE_NS = (8000, 9600, 12000, 10400)
PIPE_SIDS = [0, 3, 7, 1]


def speech(n, seed, scale=1.0):
    """A float32 clip for the networks' own entry points."""
    from rvcx import synthetic

    return (synthetic.speech_like(n, seed=seed) * scale).astype(np.float32)


def clip(n, seed):
    """A float64 clip for the pipeline."""
    from rvcx import synthetic

    return synthetic.speech_like(n, seed=seed)


def noise_for(engine, audios, opts, seed):
    """Injected noise in the batch layouts, T = the longest row's frames; row b consumes ez[b, :, :T_b], es[b, :T_b upp]."""
    Ts = [engine.pipeline_frames(len(a), opts) for a in audios]
    rng = np.random.default_rng(seed)
    ez = rng.standard_normal((len(audios), 192, max(Ts))).astype(np.float32)
    es = rng.standard_normal((len(audios), max(Ts) * engine.upp)).astype(np.float32)
    return Ts, ez, es


def cents_apart(f, g):
    v = g > 0
    return float(np.abs(1200.0 * np.log2(f[v] / g[v])).max()) if v.any() else 0.0


def compare_row(name, y, y1, f0=None, f1=None):
    """One row of a ragged-f0 pass against the single-utterance run: spectrogram correlation > 0.999, max difference
    < 5e-3 of the peak (test_pipeline_batch_matches_single's bars) and, where the caller has the rows' f0, the same
    voicing and f0 within 0.1 cent on every frame (the bound derived in test_gpu_rmvpe_ragged.py's
    check_rows_vs_single). Returns the failures."""
    from oracle.metrics import spectrogram_correlation

    assert y.shape == y1.shape, (name, y.shape, y1.shape)
    corr = spectrogram_correlation(y, y1)
    diff = float(np.abs(y - y1).max()) / max(float(np.abs(y1).max()), 1e-6)
    same_voicing, cents = True, 0.0
    if f0 is not None:
        assert f0.shape == f1.shape, (name, f0.shape, f1.shape)
        same_voicing = np.array_equal(f0 > 0, f1 > 0)
        both = (f0 > 0) & (f1 > 0)
        cents = cents_apart(f0[both], f1[both])
    print(f"\n{name}: corr {corr:.6f} max diff / peak {diff:.3e} f0 {cents:.5f} cent same voicing {same_voicing}")
    return [] if (corr > 0.999 and diff < 5e-3 and same_voicing and cents <= 0.1) else [
        f"{name}: corr {corr:.6f} diff {diff:.3e} f0 {cents:.4f} cent, same voicing {same_voicing}"]


def check_rows_vs_single(engine, audios, sids, seed, batch_kw, single_kw, judge=None, **kw):
    """Every row of one pipeline_batch_v pass (options kw + batch_kw) against pipeline_ex (kw + single_kw) on that
    utterance alone with its slice of the injected noise: equal shape and n_out, then compare_row, or the caller's own
    bars judge(b, name, y, y1, f0, f1), which returns row b's failures. The device status is clean at the end."""
    engine.set_pipeline_highpass()
    opts = engine.pipeline_opts(**kw, **batch_kw)
    upp = engine.upp
    Ts, ez, es = noise_for(engine, audios, opts, seed)
    ys, f0s = engine.pipeline_batch_v(audios, opts, sids=sids, eps_z=ez, eps_src=es, want_f0=True)
    ys, f0s = [engine.host(y) for y in ys], [engine.host(f) for f in f0s]
    failed = []
    for b, a in enumerate(audios):
        o1 = engine.pipeline_opts(sid=sids[b], **kw, **single_kw)
        y1, f1 = engine.pipeline_ex(a, o1, eps_z=np.ascontiguousarray(ez[b, :, :Ts[b]]).reshape(-1),
                                    eps_src=es[b, :Ts[b] * upp], want_f0=True)
        y1, f1 = engine.host(y1), engine.host(f1)
        assert ys[b].shape == y1.shape == (Ts[b] * upp - 2 * int(opts.t_pad_tgt),), (b, ys[b].shape, y1.shape)
        name = f"row {b} n={len(a)} T={Ts[b]}"
        failed += judge(b, name, ys[b], y1, f0s[b], f1) if judge else compare_row(name, ys[b], y1, f0s[b], f1)
    engine.check_device_status()
    assert not failed, "; ".join(failed)
