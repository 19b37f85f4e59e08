"""What the voice-bank tests share (test_gpu_voice_bank.py, test_gpu_stream_voices.py, test_gpu_batch_voices.py): the
seeded voices, a small IVF index per voice, engines that hold several of them, and the stream-group helpers and oracle
bars of test_gpu_stream_slots.py with the voice as a parameter. A plain module, like ragged_rows.py: no test module
imports another.

Voices are synthetic.synth_state(seed) at SYNTH_48K_V2. Two of them tell each other apart clearly (on the CPU oracle,
synth_infer at T = 87: pairwise spectrogram correlation 0.68-0.77, maximum difference 0.93-1.35 of the peak), so a row
converted with the wrong voice misses every bar here by two orders of magnitude; `assert_separated` holds a test's own
voices to that before the test trusts its bars."""
import numpy as np
import torch

BLOCK = 12288  # read_chunk_size 96: 87 frames, 12288-sample blocks
FRAMES = 87
WINDOW = 480 + 12288 + 4800  # the model samples SOLA reads: search + block + crossfade (the generator's output window)
RVCX_E_INVALID, RVCX_E_SHAPE, RVCX_E_STATE = -1, -2, -5
# voice seeds: A is the session fixture synth_w's
SEED_A, SEED_B, SEED_C, SEED_X = 2, 3, 21, 22

_W, _IDX = {}, {}


def weights(seed, cfg=None):
    """normalize_state(synthetic.synth_state(seed[, cfg])), built once and never modified."""
    key = (seed, repr(cfg))
    if key not in _W:
        from rvcx import synthetic
        from rvcx.weights import normalize_state

        _W[key] = normalize_state(synthetic.synth_state(seed) if cfg is None else synthetic.synth_state(seed, cfg))
    return _W[key]


def index_for(hubert_w, seed):
    """A small IVF index of a voice's own: the oracle HuBERT's features of a 2 s training clip drawn from the voice's
    seed (as test_gpu_stream_slots.py builds its one index) -> (the oracle's index, its faiss file image)."""
    if seed not in _IDX:
        from oracle import hubert as ohubert
        from oracle import ivf
        from rvcx import synthetic
        from rvcx.config import HUBERT_BASE

        train = synthetic.speech_like(16000 * 2, seed=300 + seed).astype(np.float32)
        with torch.no_grad():
            feats = ohubert.hubert_forward(hubert_w, HUBERT_BASE, torch.from_numpy(train).view(1, -1), "v2")[0].numpy()
        ix = ivf.build_ivfflat(feats, nlist=6, nprobe=1)
        _IDX[seed] = (ix, ivf.write_ivfflat(ix))
    return _IDX[seed]


def bank_engine(hubert_w, rmvpe_w, seeds, indexed=True):
    """An Engine with HuBERT and RMVPE and one voice per seed: voice 0 the first seed (loaded the old way), the others
    added after it in order; each with its own index unless indexed is False. -> (engine, ids by seed)."""
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine

    e = Engine(0)
    e.load_synth(weights(seeds[0]), SYNTH_48K_V2)
    e.load_hubert(hubert_w)
    e.load_rmvpe(rmvpe_w)
    if indexed:
        e.index_load(index_for(hubert_w, seeds[0])[1])
    ids = {seeds[0]: 0}
    for s in seeds[1:]:
        ids[s] = e.add_voice(weights(s), SYNTH_48K_V2, index=index_for(hubert_w, s)[1] if indexed else None)
    assert e.voice == 0
    return e, ids


def assert_separated(name, ya, yb):
    """The same row under two voices: spectrogram correlation < 0.9 and a difference > 0.5 of the peak."""
    from oracle.metrics import spectrogram_correlation

    corr = spectrogram_correlation(ya, yb)
    diff = float(np.abs(ya - yb).max()) / max(float(np.abs(ya).max()), float(np.abs(yb).max()), 1e-6)
    print(f"\n{name}: two voices on one row: corr {corr:.4f} max diff / peak {diff:.3f}")
    assert corr < 0.9 and diff > 0.5, (name, corr, diff)


def group(eng, B, voices=None, sids=None):
    from rvcx.realtime import StreamGroup

    grp = StreamGroup(eng, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=list(range(B)) if sids is None else sids, voices=voices)
    assert grp.geometry["block48"] == BLOCK and grp.geometry["frames"] == FRAMES
    return grp


def blocks(n, seed):
    """n consecutive blocks of one speech-like signal, [n, BLOCK]."""
    from rvcx import synthetic

    return synthetic.speech_like(BLOCK * n, seed=seed, sr=48000).astype(np.float32).reshape(n, BLOCK)


def noise(rng, B):
    """Injected noise of one hop, indexed by slot: (eps_z [B, inter, frames], eps_src [B, frames * upp])."""
    from rvcx.config import SYNTH_48K_V2

    I, upp = SYNTH_48K_V2.inter_channels, SYNTH_48K_V2.upp
    return (rng.standard_normal((B, I, FRAMES)).astype(np.float32),
            rng.standard_normal((B, FRAMES * upp)).astype(np.float32))


def hop(eng, grp, x, opts, ez, es, active=None):
    """One hop -> (out, vol, offs, model rows [active rows, frames * upp] in compact-row order) as numpy copies."""
    out, vol = grp.process(x, opts, eps_z=ez, eps_src=es, active=active)
    rows = grp.n_streams if active is None else int(sum(bool(a) for a in active))
    model = eng.rt_model_rows(grp, rows, False)
    torch.cuda.synchronize()
    return (out.cpu().numpy().copy(), vol.cpu().numpy().copy(), grp.offs.cpu().numpy().copy(),
            model.cpu().numpy().copy())


def compact_rows(voices, active=None):
    """slot -> compact row of a hop, as the library orders them: the voices by their lowest active slot, the slots of a
    voice in order (the host-side restatement the tests index model rows with)."""
    slots = [b for b in range(len(voices)) if active is None or active[b]]
    first = {}
    for b in slots:
        first.setdefault(voices[b], len(first))
    order = sorted(slots, key=lambda b: first[voices[b]])
    return {b: r for r, b in enumerate(order)}


def oracle_changer(synth_w, hubert_w, rmvpe_w, sid, index=None):
    from oracle.realtime import OracleVoiceChanger
    from rvcx.config import HUBERT_BASE, RMVPE_CFG, SYNTH_48K_V2

    return OracleVoiceChanger(synth_w, SYNTH_48K_V2, hubert_w, HUBERT_BASE, rmvpe_w, RMVPE_CFG, read_chunk_size=96,
                              silent_threshold=-90.0, sid=sid, index=index)


class Bars:
    """The oracle bars of test_gpu_stream.py, gathered over the hops of one test: vol rel <= 1e-5, per-hop output
    spectrogram correlation > 0.99, SOLA offsets equal on >= 75 % of the non-silent hops."""

    def __init__(self):
        self.same, self.n = 0, 0

    def hop(self, orc, x, ez, es, kw, out, vol, off, tag):
        from oracle.metrics import spectrogram_correlation

        it = iter([torch.from_numpy(ez[None]), torch.from_numpy(es[None])])
        orc.noise_fn = lambda shape, which, it=it: next(it)
        ref, rvol = orc.on_request(x.copy(), **kw)
        print(tag, "vol", vol, rvol, "offs", off, orc.last.get("sola_offset"))
        assert abs(vol - rvol) <= 1e-5 * max(rvol, 1e-12), (tag, vol, rvol)
        if not np.any(ref):
            np.testing.assert_array_equal(out, ref)
            return
        self.n += 1
        self.same += int(off == orc.last["sola_offset"])
        corr = spectrogram_correlation(out, ref)
        print(tag, "corr", corr)
        assert corr > 0.99, (tag, corr)

    def finish(self):
        assert self.same >= 0.75 * self.n, (self.same, self.n)
