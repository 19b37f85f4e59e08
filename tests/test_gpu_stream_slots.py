"""Stream groups as a multi-tenant object (rvcx.realtime.StreamGroup through rvcx_rt_process_v / rvcx_rt_reset_stream):
one RtOpts per slot, slots that sit a hop out, and the reset of one slot.

Two kinds of bar. Against the oracle restatement of rvc/realtime (oracle/realtime.py, one OracleVoiceChanger per
stream with that stream's own on_request arguments) the bars are those of test_gpu_stream.py: vol rel <= 1e-5, per-hop
output spectrogram correlation > 0.99, SOLA offsets equal on >= 75 % of the non-silent hops. Between two device runs
the bar is bit equality, and every such comparison pairs hops that ran the same number of active rows with the stream
in the same compact position (a batch of another size may pick another GEMM split, test_gpu_stream_fcpe.py).

Geometry of the existing stream tests: read_chunk_size 96, crossfade 0.1, extra 0.5 -> 87 frames, 12288-sample blocks.
Noise is always injected and indexed by slot."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCK = 12288
RVCX_E_INVALID, RVCX_E_STATE = -1, -5

# the three option sets of the mixed group, as keyword arguments of StreamGroup.opts and OracleVoiceChanger.on_request
MIXED = (
    dict(f0_up_key=7, protect=0.33, index_rate=0.6),
    dict(f0_autotune=True, f0_autotune_strength=0.7, index_rate=0.0, volume_envelope=0.4),
    dict(f0_up_key=-3, proposed_pitch=True, proposed_pitch_threshold=200.0, index_rate=1.0),
)


@pytest.fixture(scope="module")
def index(hubert_w):
    """A small IVF index over the oracle HuBERT's features of a training clip (as test_gpu_index.py builds it)."""
    from oracle import hubert as ohubert
    from oracle import ivf
    from rvcx import synthetic
    from rvcx.config import HUBERT_BASE

    train = synthetic.speech_like(16000 * 2, seed=31).astype(np.float32)
    with torch.no_grad():
        feats = ohubert.hubert_forward(hubert_w, HUBERT_BASE, torch.from_numpy(train).view(1, -1), "v2")[0].numpy()
    return ivf.build_ivfflat(feats, nlist=6, nprobe=1)


@pytest.fixture(scope="module")
def eng(synth_w, hubert_w, rmvpe_w, index):
    """An engine of this module's own (the index must not leak into the session engine's default opts)."""
    from oracle import ivf
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine

    e = Engine(0)
    e.load_synth(synth_w, SYNTH_48K_V2)
    e.load_hubert(hubert_w)
    e.load_rmvpe(rmvpe_w)
    e.index_image = ivf.write_ivfflat(index)  # kept to load it back after the no-index check
    e.index_load(e.index_image)
    yield e
    e.close()


def _group(eng, B, sids=None):
    from rvcx.realtime import StreamGroup

    grp = StreamGroup(eng, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=list(range(B)) if sids is None else sids)
    assert grp.geometry["block48"] == BLOCK and grp.geometry["frames"] == 87
    return grp


def _blocks(n, seed):
    """n consecutive blocks of one speech-like signal, [n, BLOCK]."""
    from rvcx import synthetic

    return synthetic.speech_like(BLOCK * n, seed=seed, sr=48000).astype(np.float32).reshape(n, BLOCK)


def _noise(rng, B):
    from rvcx.config import SYNTH_48K_V2

    I, T, upp = SYNTH_48K_V2.inter_channels, 87, SYNTH_48K_V2.upp
    return (rng.standard_normal((B, I, T)).astype(np.float32), rng.standard_normal((B, T * upp)).astype(np.float32))


def _hop(grp, x, opts, ez, es, active=None):
    """One hop -> (out, vol, offs) as numpy copies."""
    out, vol = grp.process(x, opts, eps_z=ez, eps_src=es, active=active)
    torch.cuda.synchronize()
    return out.cpu().numpy().copy(), vol.cpu().numpy().copy(), grp.offs.cpu().numpy().copy()


def _oracle(synth_w, hubert_w, rmvpe_w, sid, index=None):
    from oracle.realtime import OracleVoiceChanger
    from rvcx.config import HUBERT_BASE, RMVPE_CFG, SYNTH_48K_V2

    return OracleVoiceChanger(synth_w, SYNTH_48K_V2, hubert_w, HUBERT_BASE, rmvpe_w, RMVPE_CFG, read_chunk_size=96,
                              silent_threshold=-90.0, sid=sid, index=index)


class _Bars:
    """The oracle bars of test_gpu_stream.py, gathered over the hops of one test."""

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


@pytest.fixture(scope="module")
def mixed_run(eng):
    """The mixed group (B = 3, one option set per stream) over 3 hops: inputs, noise and results, computed once."""
    B, hops = 3, 3
    audio = np.stack([_blocks(hops, 60 + b) for b in range(B)])  # [B, hops, BLOCK]
    rng = np.random.default_rng(7)
    noise = [_noise(rng, B) for _ in range(hops)]
    grp = _group(eng, B)
    opts = [grp.opts(**kw) for kw in MIXED]
    assert [o.index_rate for o in opts] == [0.6, 0.0, 1.0]
    res = [_hop(grp, audio[:, h], opts, *noise[h]) for h in range(hops)]
    grp.close()
    return dict(audio=audio, noise=noise, res=res)


def test_mixed_options_equal_uniform_rows(eng, mixed_run):
    """Row i of the mixed group == row i of a B = 3 group run uniformly with option set i, bit for bit."""
    audio, noise = mixed_run["audio"], mixed_run["noise"]
    for i, kw in enumerate(MIXED):
        grp = _group(eng, 3)
        o = grp.opts(**kw)
        for h in range(3):
            out, vol, offs = _hop(grp, audio[:, h], o, *noise[h])
            mo, mv, mf = mixed_run["res"][h]
            np.testing.assert_array_equal(out[i], mo[i], err_msg=f"set {i} hop {h}")
            assert vol[i] == mv[i] and offs[i] == mf[i], (i, h, vol[i], mv[i], offs[i], mf[i])
        grp.close()
    # the three rows really ran different options: no two rows of a uniform group would differ only by their sid
    assert not np.array_equal(mixed_run["res"][2][0][0], mixed_run["res"][2][0][2])


def test_mixed_options_match_oracle(mixed_run, synth_w, hubert_w, rmvpe_w, index):
    """The mixed group against one OracleVoiceChanger per stream with that stream's arguments and index."""
    audio, noise = mixed_run["audio"], mixed_run["noise"]
    bars = _Bars()
    for b, kw in enumerate(MIXED):
        orc = _oracle(synth_w, hubert_w, rmvpe_w, b, index)
        for h in range(3):
            out, vol, offs = mixed_run["res"][h]
            bars.hop(orc, audio[b, h], noise[h][0][b], noise[h][1][b], kw, out[b], vol[b], offs[b], (b, h))
    bars.finish()


def test_one_opts_equals_list_of_it(eng):
    """process(x, one_opts) and process(x, [one_opts] * B) on two fresh groups are bit-identical, and so is the C entry
    point that takes one rvcx_rt_opts (rvcx_rt_process) on a third."""
    B = 3
    audio = np.stack([_blocks(2, 70 + b) for b in range(B)])
    rng = np.random.default_rng(11)
    noise = [_noise(rng, B) for _ in range(2)]
    ga, gb, gc = _group(eng, B), _group(eng, B), _group(eng, B)
    kw = dict(f0_up_key=2, protect=0.4, index_rate=0.5, volume_envelope=0.7)
    for h in range(2):
        ra = _hop(ga, audio[:, h], ga.opts(**kw), *noise[h])
        rb = _hop(gb, audio[:, h], [gb.opts(**kw)] * B, *noise[h])
        xd, ezd, esd = (eng._dev(v, torch.float32) for v in (audio[:, h], *noise[h]))
        eng._check(eng.lib.rvcx_rt_process(eng.ctx, gc.handle, xd.data_ptr(), gc.sids, ctypes.byref(gc.opts(**kw)),
                                           ezd.data_ptr(), esd.data_ptr(), ctypes.c_uint64(0), gc.out.data_ptr(),
                                           gc.vol.data_ptr(), gc.offs.data_ptr(), eng.stream()), "rt_process")
        torch.cuda.synchronize()
        rc = (gc.out.cpu().numpy(), gc.vol.cpu().numpy(), gc.offs.cpu().numpy())
        for a, b, c in zip(ra, rb, rc):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)
        assert np.isfinite(ra[0]).all() and np.any(ra[0])
    for g in (ga, gb, gc):
        g.close()


def test_idle_slot(eng, synth_w, hubert_w, rmvpe_w):
    """A slot that sits a hop out: its input is not read, its outputs are zero, and its next hop is the one it would
    have had without the pause. The stream that did run meets the oracle bars."""
    B = 2
    a, b = _blocks(4, 80), _blocks(3, 81)
    rng = np.random.default_rng(13)
    noise = [_noise(rng, B) for _ in range(4)]
    X, Y = _group(eng, B), _group(eng, B)
    kw = dict(index_rate=0.0)
    nan = np.full(BLOCK, np.nan, np.float32)
    # X: four calls, stream 1 idle on the third
    x_in = [np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), np.stack([a[2], nan]), np.stack([a[3], b[2]])]
    x_act = [None, None, [True, False], None]
    rx = [_hop(X, x_in[h], X.opts(**kw), *noise[h], active=x_act[h]) for h in range(4)]
    # Y: three calls, stream 1 with the same three blocks and noise (X's calls 1, 2 and 4)
    ry = [_hop(Y, x_in[h], Y.opts(**kw), *noise[h]) for h in (0, 1, 3)]
    for got, want in zip(ry[2], rx[3]):
        np.testing.assert_array_equal(got[1], want[1])
    assert np.any(rx[3][0][1])
    out3, vol3, offs3 = rx[2]
    assert not np.any(out3[1]) and vol3[1] == 0 and offs3[1] == 0
    assert np.isfinite(out3[0]).all()
    # stream 0 of X against the oracle, the third call (alone in its batch) included
    orc = _oracle(synth_w, hubert_w, rmvpe_w, 0)
    bars = _Bars()
    for h in range(3):
        out, vol, offs = rx[h]
        bars.hop(orc, a[h], noise[h][0][0], noise[h][1][0], kw, out[0], vol[0], offs[0], ("idle", h))
    bars.finish()
    X.close()
    Y.close()


def test_compaction_with_gaps(eng, synth_w, hubert_w, rmvpe_w, index):
    """B = 4 with slots 0 and 2 idle on the middle hop: every stream meets the oracle bars on each hop it took part
    in; a hop with no active slot returns zeros and changes nothing that follows."""
    B = 4
    sids = [0, 2, 1, 3]
    kws = [dict(index_rate=0.0), dict(f0_up_key=5, protect=0.3, index_rate=0.7), dict(index_rate=0.0),
           dict(f0_up_key=-4, volume_envelope=0.5, index_rate=0.0)]
    audio = np.stack([_blocks(4, 90 + s) for s in range(B)])
    rng = np.random.default_rng(17)
    noise = [_noise(rng, B) for _ in range(4)]
    active = [None, [False, True, False, True], None, None]
    P, Q = _group(eng, B, sids), _group(eng, B, sids)
    rp = []
    for h in range(3):
        x = audio[:, h].copy()
        if active[h] is not None:
            x[[0, 2]] = np.nan
        rp.append(_hop(P, x, [P.opts(**kw) for kw in kws], *noise[h], active=active[h]))
    rq = [_hop(Q, audio[:, h], [Q.opts(**kw) for kw in kws], *noise[h], active=active[h]) for h in range(3)]
    # nobody active: zeros, and the hop after it equals that of a group that never saw the empty call
    out, vol, offs = _hop(P, np.full((B, BLOCK), np.nan, np.float32), [P.opts(**kw) for kw in kws], *noise[3],
                          active=[False] * B)
    assert not np.any(out) and not np.any(vol) and not np.any(offs)
    last_p = _hop(P, audio[:, 3], [P.opts(**kw) for kw in kws], *noise[3])
    last_q = _hop(Q, audio[:, 3], [Q.opts(**kw) for kw in kws], *noise[3])
    for h in range(3):
        for got, want in zip(rp[h], rq[h]):
            np.testing.assert_array_equal(got, want)
    for got, want in zip(last_p, last_q):
        np.testing.assert_array_equal(got, want)
    assert np.isfinite(last_p[0]).all() and np.any(last_p[0])
    out, vol, offs = rp[1]
    assert not np.any(out[[0, 2]]) and not np.any(vol[[0, 2]]) and not np.any(offs[[0, 2]])
    bars = _Bars()
    for s in range(B):
        orc = _oracle(synth_w, hubert_w, rmvpe_w, sids[s], index if kws[s]["index_rate"] > 0 else None)
        for h in range(3):
            if active[h] is not None and not active[h][s]:
                continue
            out, vol, offs = rp[h]
            bars.hop(orc, audio[s, h], noise[h][0][s], noise[h][1][s], kws[s], out[s], vol[s], offs[s], (s, h))
    bars.finish()
    P.close()
    Q.close()


def test_slot_reset(eng):
    """reset(stream=1) between hops: stream 1 continues as a fresh group's stream 1, stream 0 as if nothing happened."""
    B = 2
    a, b = _blocks(4, 100), _blocks(4, 101)
    rng = np.random.default_rng(19)
    noise = [_noise(rng, B) for _ in range(4)]
    x = [np.stack([a[h], b[h]]) for h in range(4)]
    kw = dict(f0_up_key=3, index_rate=0.4)
    P, N, F = _group(eng, B), _group(eng, B), _group(eng, B)
    rp = []
    for h in range(4):
        if h == 2:
            P.reset(stream=1)
        rp.append(_hop(P, x[h], P.opts(**kw), *noise[h]))
    rn = [_hop(N, x[h], N.opts(**kw), *noise[h]) for h in range(4)]
    rf = [_hop(F, x[h], F.opts(**kw), *noise[h]) for h in (2, 3)]
    for h in range(4):
        for got, want in zip(rp[h], rn[h]):
            np.testing.assert_array_equal(got[0], want[0], err_msg=f"stream 0 hop {h}")
    for k, h in enumerate((2, 3)):
        for got, want in zip(rp[h], rf[k]):
            np.testing.assert_array_equal(got[1], want[1], err_msg=f"stream 1 hop {h}")
    # the reset did something: the never-reset group's stream 1 still carries its first two hops
    assert not np.array_equal(rp[2][0][1], rn[2][0][1])
    for g in (P, N, F):
        g.close()


def test_errors_leave_the_group_usable(eng):
    from rvcx import _lib
    from rvcx.realtime import hop_arguments

    B = 2
    grp = _group(eng, B)
    rng = np.random.default_rng(23)
    x = np.stack([_blocks(1, 110)[0], _blocks(1, 111)[0]])
    ez, es = _noise(rng, B)
    ok = grp.opts(index_rate=0.0)
    first = _hop(grp, x, ok, ez, es)
    lowp = grp.opts(index_rate=0.0, gen_precision="fp16")
    with pytest.raises(ValueError):
        grp.process(x, [ok, lowp], eps_z=ez, eps_src=es)
    # an idle slot's precision does not count
    hop_arguments(B, [ok, lowp], [True, False])
    # the library refuses it too
    arr = (_lib.RtOpts * B)()
    for i, o in enumerate((ok, lowp)):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(o), ctypes.sizeof(_lib.RtOpts))
    xd, ezd, esd = (eng._dev(v, torch.float32) for v in (x, ez, es))
    rc = eng.lib.rvcx_rt_process_v(eng.ctx, grp.handle, xd.data_ptr(), grp.sids, arr, None, ezd.data_ptr(),
                                   esd.data_ptr(), ctypes.c_uint64(0), grp.out.data_ptr(), grp.vol.data_ptr(),
                                   grp.offs.data_ptr(), eng.stream())
    assert rc == RVCX_E_INVALID
    with pytest.raises(ValueError):
        grp.process(x, [ok] * (B + 1), eps_z=ez, eps_src=es)
    with pytest.raises(ValueError):
        grp.process(x, ok, eps_z=ez, eps_src=es, active=[True])
    with pytest.raises(ValueError):
        grp.reset(stream=B)
    assert eng.lib.rvcx_rt_reset_stream(eng.ctx, grp.handle, B, eng.stream()) == RVCX_E_INVALID
    # index_rate > 0 on an active stream with no index loaded
    eng.index_unload()
    try:
        want = grp.opts()
        want.index_rate = 0.5
        with pytest.raises(_lib.RvcxError) as ei:
            grp.process(x, [ok, want], eps_z=ez, eps_src=es)
        assert ei.value.code == RVCX_E_STATE
        grp.process(x, [ok, want], eps_z=ez, eps_src=es, active=[True, False])  # idle: its index_rate is ignored
        torch.cuda.synchronize()
    finally:
        eng.index_load(eng.index_image)
    # none of the refused calls touched the state: a fresh group fed only the accepted hops gives the same audio
    ref = _group(eng, B)
    for got, want_ in zip(first, _hop(ref, x, ref.opts(index_rate=0.0), ez, es)):
        np.testing.assert_array_equal(got, want_)
    ref.process(x, ref.opts(index_rate=0.0), eps_z=ez, eps_src=es, active=[True, False])
    for got, want_ in zip(_hop(grp, x, ok, ez, es), _hop(ref, x, ref.opts(index_rate=0.0), ez, es)):
        np.testing.assert_array_equal(got, want_)
        assert np.isfinite(got).all() and np.any(got)
    grp.close()
    ref.close()
