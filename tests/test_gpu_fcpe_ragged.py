"""FCPE over a batch of rows of different lengths in one pass (rvcx_fcpe_batch_v), against the float64 restatement
(tests/fcpe_ref.py) on each row alone and against the single-row call, the ragged Performer attention at kernel level,
and the ragged pipeline with it (rvcx_pipeline_opts.f0_method 5). The model is the seeded 2-layer, 512-channel model of
tests/golden/fcpe_l2.npz; the threshold is 0.5.

The batch: synthetic.speech_like(n, seed) for

        n   seed     F
     1000     70     7   below one 16-row time tile, shorter than the k = 31 kernel
     2400     71    16   exactly one tile
    13920     72    88   the realtime buffer
    20480     73   129   two attention slabs, the second holding one row
    48000     74   301   three slabs

so rows of 1, 2 and 3 slabs share one launch. It runs in the given order and reversed.

A frame is near-tied when its float64 top-2 margin is below 2 K gap or its maximum within K gap of the threshold
(K = 8, gap the row's own fp32-vs-float64 distance). On the CPU the reference gives 0 / 7, 0 / 16, 0 / 88, 0 / 129 and
1 / 301 such frames (gaps 5.9e-7 .. 1.2e-5; the one frame has its maximum 6.4e-5 from 0.5); the voiced share is
0.40 .. 0.57 per row and the peak sits in 6 .. 86 distinct bins. At most 2 % of a row's frames may be near-tied
(test_gpu_fcpe.py's cap): the `rows` fixture asserts it on the margins it computes.
"""
import ctypes

import numpy as np
import pytest
import torch

import fcpe_ref as fr
import parity_anchor as pa
import ragged_rows
from conftest import golden
from fcpe_ref import ATTN_D as D, ATTN_H as H, ATTN_M as M, attention_operands as _attention_operands
from ragged_rows import PIPE_NS, PIPE_SIDS, SHORT_PAD, cents_apart, clip, compare_row, speech

pytestmark = pytest.mark.gpu

NS = (1000, 2400, 13920, 20480, 48000)
FS = (7, 16, 88, 129, 301)
THR = 0.5


@pytest.fixture(scope="module")
def model(engine):
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, fcpe_sizes

    g = golden("fcpe_l2.npz")
    cfg = synthetic.fcpe_config(int(g["n_layers"]), int(g["n_chans"]))
    raw = synthetic.fcpe_state(int(g["seed"]), int(g["n_layers"]), int(g["n_chans"]))
    engine.load_fcpe(raw, cfg)
    return dict(z=fcpe_sizes(cfg), w=check_fcpe_state(raw, cfg), raw=raw, cfg=cfg)


@pytest.fixture(scope="module")
def rows(model):
    """Per row: the audio, the float64 salience of that row alone, its fp32 gap and the near-tied frames (computed once
    for all tests, never modified)."""
    out = []
    for b, n in enumerate(NS):
        audio = speech(n, 70 + b)
        a = torch.from_numpy(audio)
        ref, gap = pa.anchor(lambda dt, a=a: fr.salience_from_audio(pa.weights(model["w"], dt), model["z"],
                                                                    a.to(dt)))["out"]
        assert ref.shape == (FS[b], 360)
        srt = np.sort(ref, axis=1)
        e = pa.K * max(gap, pa.ULP32)
        near = (srt[:, -1] - srt[:, -2] < 2 * e) | (np.abs(srt[:, -1] - THR) <= e)
        assert near.mean() <= 0.02, f"n={n}: {int(near.sum())} of {FS[b]} frames near-tied at K gap = {e:.2e}"
        ref.setflags(write=False)
        out.append((audio, ref, gap, near))
    return out


@pytest.fixture(scope="module")
def single(engine, model, rows):
    """engine.fcpe on every row alone: (f0, salience)."""
    return [tuple(engine.host(x) for x in engine.fcpe(a, THR, want_salience=True)) for a, _, _, _ in rows]


def run_rows(engine, audios):
    f0s, sals = engine.fcpe_batch_v(audios, THR, want_salience=True)
    return [engine.host(x) for x in f0s + sals]


# ----------------------------------------------------------------- every row against float64 and the single run
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_ragged_fcpe_vs_fp64_and_single(engine, model, rows, single, order):
    """Per row: the salience within K gaps (absolute) of float64 on that row alone, shapes (F_b, 360). f0 is the
    local_argmax decode of the device's own salience row (voicing exact, rtol 2e-6, fp32-valued: the bars of
    test_gpu_fcpe_batch.py). Against engine.fcpe on the row alone, on every frame that is not near-tied: the same
    voicing, the same peak bin, and f0 within 0.1 cent. That bound is compare_row's derivation with FCPE's numbers:
    f0 = 10 * 2^(c / 1200) with c the salience-weighted mean of nine bins of the cent table, 19.8 cents apart, so
    sum |bin - mean| <= 2 (1 + 2 + 3 + 4) 20 = 400 cents; two fp32 evaluations of the salience, each within 5e-5 of
    float64 (the largest K gap here is 9.6e-5 for the two together), on weights whose sum is at least the voiced
    maximum 0.5, move c by at most 2 * 5e-5 * 400 / 0.5 = 0.08 cent."""
    idx = list(range(len(NS))) if order == "given" else list(reversed(range(len(NS))))
    f0s, sals = engine.fcpe_batch_v([rows[i][0] for i in idx], THR, want_salience=True)
    assert len(f0s) == len(sals) == len(idx)
    cent = torch.from_numpy(model["w"]["cent_table"])
    failed = []
    for f0, sal, i in zip(f0s, sals, idx):
        _, ref, gap, near = rows[i]
        f0, sal = engine.host(f0), engine.host(sal)
        assert f0.shape == (FS[i],) and sal.shape == (FS[i], 360), (NS[i], f0.shape, sal.shape)
        try:
            pa.check(f"fcpe_batch_v {order} row n={NS[i]} vs fp64", sal, ref, gap, pa.K, absolute=True)
            want = fr.decode(torch.from_numpy(sal), cent, THR).numpy()
            assert np.array_equal(f0 > 0, want > 0), "voicing is not the decode's of the device's own salience"
            np.testing.assert_allclose(f0, want, rtol=2e-6, atol=0)
            assert np.array_equal(f0.astype(np.float32).astype(np.float64), f0), "f0 is not fp32-valued"
            f1, s1 = single[i]
            ok = ~near
            assert np.array_equal(f0[ok] > 0, f1[ok] > 0), "voicing differs from the single run's"
            assert np.array_equal(sal.argmax(1)[ok], s1.argmax(1)[ok]), "peak bin differs from the single run's"
            c = cents_apart(f0[ok], f1[ok])
            print(f"fcpe_batch_v {order} row n={NS[i]} vs single: {c:.5f} cent, {int(near.sum())} frames exempt, "
                  f"salience max diff {float(np.abs(sal - s1).max()):.2e}")
            assert c <= 0.1, f"f0 {c:.4f} cent from the single run's"
        except AssertionError as e:
            failed.append(f"n={NS[i]}: {e}")
    engine.check_device_status()
    assert not failed, "; ".join(failed)


# ----------------------------------------------------------------- independence
def test_row_is_independent_of_its_neighbours(engine, model, rows):
    """Row n = 20480 (two slabs) between rows of 1000 and 48000 samples: with the neighbours replaced by other seeds and
    scales of the same lengths, its salience and f0 are bit-identical, first, in the middle and last; the neighbours'
    own rows differ."""
    mine = rows[3][0]
    a = {1000: speech(1000, 70), 48000: speech(48000, 74)}
    b = {1000: speech(1000, 91, 2.5), 48000: speech(48000, 93, 0.1)}
    for pos, lens in ((0, (20480, 1000, 48000)), (1, (48000, 20480, 1000)), (2, (1000, 48000, 20480))):
        r1 = run_rows(engine, [mine if n == 20480 else a[n] for n in lens])
        r2 = run_rows(engine, [mine if n == 20480 else b[n] for n in lens])
        for k in range(3):
            same = np.array_equal(r1[k], r2[k]) and np.array_equal(r1[3 + k], r2[3 + k])
            assert same == (k == pos), (pos, k)
        assert np.isfinite(r1[3 + pos]).all()
    engine.check_device_status()


# ----------------------------------------------------------------- stale memory
def test_stale_scratch_does_not_reach_a_row(engine, model, rows):
    """The call inside a caller-owned arena full of 0xFF (NaN bit patterns), sized by rvcx_workspace_bytes under
    f0_method 5 for as many rows of the longest length: every row's f0 and salience finite and the free run's bits.
    Nothing past a row's end (another row's frames, the pad rows of its own slot, scratch no kernel wrote) reaches it."""
    t = engine.torch
    audios = [rows[i][0] for i in (2, 4, 0, 3, 1)]
    free = run_rows(engine, audios)
    again = run_rows(engine, audios)
    assert all(np.array_equal(a, b) for a, b in zip(free, again))
    engine.set_pipeline_highpass()
    opts = engine.pipeline_opts(f0_method=5, fcpe_threshold=THR, **SHORT_PAD)
    arena = t.empty(engine.workspace_bytes(max(NS), len(NS), opts), dtype=t.uint8, device=engine.device)
    engine.set_workspace(arena)
    try:
        arena.fill_(0xFF)
        held = run_rows(engine, audios)
    finally:
        engine.set_workspace(None)
    for a, b in zip(free, held):
        assert np.isfinite(b).all() and np.array_equal(a, b)
    engine.check_device_status()


SENTINEL = -7.0


def run_rows_c(engine, audios, lda, ldf, ld_sal):
    """rvcx_fcpe_batch_v itself on buffers this test stages: NaN past every row's end in d_audio (rows lda samples
    apart), f0 rows ldf and salience rows ld_sal frames apart, both pre-filled with SENTINEL. Returns the whole f0
    [B, ldf] and salience [B, ld_sal, 360] buffers and F_out."""
    t = engine.torch
    ns = [len(a) for a in audios]
    B = len(ns)
    a = t.full((B, lda), float("nan"), dtype=t.float32, device=engine.device)
    for b, r in enumerate(audios):
        a[b, : ns[b]] = t.as_tensor(r, dtype=t.float32)
    f0 = t.full((B, ldf), SENTINEL, dtype=t.float64, device=engine.device)
    sal = t.full((B, ld_sal, 360), SENTINEL, dtype=t.float32, device=engine.device)
    F_arr = (ctypes.c_int64 * B)()
    engine._check(engine.lib.rvcx_fcpe_batch_v(engine.ctx, a.data_ptr(), (ctypes.c_int64 * B)(*ns), lda, B, THR, 0,
                                               f0.data_ptr(), ldf, F_arr, sal.data_ptr(), ld_sal, engine.stream()),
                  "fcpe_batch_v")
    return engine.host(f0), engine.host(sal), [int(v) for v in F_arr]


@pytest.mark.parametrize("equal", [False, True])
def test_wide_strides_and_nothing_written_past_a_row(engine, model, rows, equal):
    """lda, ldf and ld_sal_frames larger than the longest row needs, NaN in d_audio past every row's end and a
    sentinel in the outputs: the rows are the tight call's bits, and from F_b on the sentinel still stands. With equal
    lengths this is the equal-length pass's strided copy-out."""
    audios = [speech(13920, 80 + b) for b in range(3)] if equal else [rows[i][0] for i in (1, 4, 2)]
    tight = run_rows(engine, audios)
    B, F = len(audios), max(len(a) for a in audios) // 160 + 1
    f0, sal, Fv = run_rows_c(engine, audios, lda=max(len(a) for a in audios) + 37, ldf=F + 5, ld_sal=F + 3)
    assert Fv == [len(a) // 160 + 1 for a in audios]
    for b in range(B):
        assert np.isfinite(f0[b, : Fv[b]]).all() and np.isfinite(sal[b, : Fv[b]]).all()
        assert np.array_equal(f0[b, : Fv[b]], tight[b]) and np.array_equal(sal[b, : Fv[b]], tight[B + b])
        assert (f0[b, Fv[b]:] == SENTINEL).all() and (sal[b, Fv[b]:] == SENTINEL).all(), f"row {b} written past F_b"
    engine.check_device_status()


# ----------------------------------------------------------------- equal lengths and single rows
def test_equal_lengths_and_single_rows_take_the_existing_paths(engine, model):
    """Three rows of 13920 samples are fcpe_batch's bits, one row is engine.fcpe's, and three rows of 400 (the mel's
    zero-padding branch, which only equal lengths may take) are fcpe_batch's."""
    for n in (13920, 400):
        audio = np.stack([speech(n, 80 + b, s) for b, s in enumerate((1.0, 0.3, 2.0))])
        f_eq, s_eq = (engine.host(x) for x in engine.fcpe_batch(audio, THR, want_salience=True))
        got = run_rows(engine, list(audio))
        for b in range(3):
            assert np.array_equal(got[b], f_eq[b]) and np.array_equal(got[3 + b], s_eq[b]), (n, b)
    one = run_rows(engine, [audio[1]])
    f1, s1 = (engine.host(x) for x in engine.fcpe(audio[1], THR, want_salience=True))
    assert np.array_equal(one[0], f1) and np.array_equal(one[1], s1)
    a = speech(13920, 81, 0.3)
    one = run_rows(engine, [a])
    f1, s1 = (engine.host(x) for x in engine.fcpe(a, THR, want_salience=True))
    assert np.array_equal(one[0], f1) and np.array_equal(one[1], s1)
    engine.check_device_status()


# ----------------------------------------------------------------- refusals
def call_v(engine, ns, lda, B, ldf):
    """rvcx_fcpe_batch_v itself on a zero buffer of B x lda samples."""
    t = engine.torch
    a = t.zeros((max(B, 1), lda), dtype=t.float32, device=engine.device)
    f0 = t.empty((max(B, 1), max(ldf, 1)), dtype=t.float64, device=engine.device)
    n_arr = (ctypes.c_int64 * max(B, 1))(*ns)
    engine._check(engine.lib.rvcx_fcpe_batch_v(engine.ctx, a.data_ptr(), n_arr, lda, B, THR, 0, f0.data_ptr(), ldf, None,
                                               None, 0, engine.stream()), "fcpe_batch_v")


def test_refusals(engine, model):
    """Each on the host, before anything is launched: the device status is clean afterwards."""
    from rvcx._lib import RvcxError

    with pytest.raises(RvcxError) as e:  # a row of the zero-padding branch among rows of different lengths
        engine.fcpe_batch_v([speech(5000, 1), speech(400, 2)], THR)
    assert e.value.code == -2
    with pytest.raises(RvcxError) as e:  # no rows
        call_v(engine, [5000], 5000, 0, 64)
    assert e.value.code == -1
    with pytest.raises(RvcxError) as e:  # f0 rows too short for the longest row's 57 frames
        call_v(engine, [5000, 9000], 9000, 2, 56)
    assert e.value.code == -6
    call_v(engine, [5000, 9000], 9000, 2, 57)
    engine.check_device_status()


# ----------------------------------------------------------------- ragged attention, kernel level
def test_ragged_attention_per_stream(engine):
    """B = 3 streams of T = 7, 94 and 301 rows in one launch set (rvcx_performer_attention_v), NaN in q, k and v from
    T_b on: each stream within K gaps of float64 on its own operands, bit-equal to the B = 1 call on them (a slab
    wholly past T_b adds exact zeros to ctx and ksum, and pass B is per row), and no output row from T_b on written."""
    Ts = (7, 94, 301)
    ops = [_attention_operands(T, 1.0, 7000 + T) for T in Ts]
    P = ops[0][3]
    q, k, v = (np.full((len(Ts), H, max(Ts), D), np.nan, np.float32) for _ in range(3))
    for b, T in enumerate(Ts):
        q[b, :, :T], k[b, :, :T], v[b, :, :T] = ops[b][:3]
    assert P.shape == (M, D)
    out = engine.performer_attention_v(q, k, v, Ts, P)
    t = torch.from_numpy
    points = []
    for b, T in enumerate(Ts):
        qb, kb, vb = ops[b][:3]
        ref64, gap = pa.anchor(lambda dt, qb=qb, kb=kb, vb=vb: fr.performer_attention(
            t(qb).to(dt), t(kb).to(dt), t(vb).to(dt), t(P).to(dt)))["out"]
        points.append((f"ragged performer T={T} stream {b}", out[b, :, :T], ref64, gap, pa.K))
        assert torch.isnan(out[b, :, T:]).all(), f"stream {b}: rows past T_b written"
        assert torch.equal(out[b, :, :T], engine.performer_attention(qb, kb, vb, P)), f"stream {b} != the B = 1 call"
    pa.check_each(points)
    assert torch.equal(engine.performer_attention_v(q, k, v, Ts, P)[2], out[2])
    engine.check_device_status()


# ----------------------------------------------------------------- the ragged pipeline with f0_method 5
PIPE_SEEDS_FCPE = (100, 200, 300, 501)
EQUAL_N, EQUAL_SEEDS = 9600, (200, 201, 202)


def pipe_clips():
    return [clip(n, s) for n, s in zip(PIPE_NS, PIPE_SEEDS_FCPE)]


def check_rows_vs_single(engine, audios, sids, seed, **kw):
    """The ragged RMVPE test's procedure (ragged_rows.check_rows_vs_single) with FCPE: pipeline_batch_v under
    f0_method 5 against pipeline_ex under f0_method 3 on each utterance alone with its slice of the injected noise, at
    compare_row's bars (spectrogram correlation > 0.999, max difference < 5e-3 of the peak, the adjusted f0 with the
    same voicing and within 0.1 cent on EVERY frame), the single run's track 20 .. 80 % voiced."""
    def judge(b, name, y, y1, f0, f1):
        assert 0.2 < float((f1 > 0).mean()) < 0.8
        return compare_row(name, y, y1, f0, f1)

    ragged_rows.check_rows_vs_single(engine, audios, sids, seed, dict(f0_method=5), dict(f0_method=3), judge, pitch=2.0,
                                     protect=0.33, fcpe_threshold=THR, **kw)


@pytest.mark.parametrize("envelope", [1.0, 0.5])
def test_ragged_f0_pipeline_matches_single(engine, model, envelope):
    """PIPE_NS with PIPE_SEEDS_FCPE: no frame is exempt, so per row the seed is the first of 100 k + j (k = 1, 2, 3, 5)
    whose input, high-passed and reflect-padded by 4800 samples as the pipeline pads it, has no near-tied frame in the
    float64 FCPE salience at threshold 0.5 (top-2 margin >= 2 K gap, maximum further than K gap from 0.5; K = 8, gap the
    restatement's own fp32-vs-float64 distance on that input). Computed on the CPU:

          n   seed     F      gap     K gap   min margin   min |top - 0.5|   voiced
       8000    100   111   2.06e-6   1.65e-5    3.68e-4       1.15e-3         0.57
       9600    200   121   7.56e-6   6.05e-5    8.43e-4       1.60e-3         0.54
      12000    300   136   7.21e-6   5.77e-5    5.10e-4       1.30e-3         0.60
      10400    501   126   9.99e-6   7.99e-5    5.98e-4       2.72e-4         0.44

    (seed 500 has one frame 1.24e-4 from the threshold at K gap 9.7e-5 and a margin of 1.55e-4 < 2 K gap.)"""
    check_rows_vs_single(engine, pipe_clips(), PIPE_SIDS, seed=3, volume_envelope=envelope, **SHORT_PAD)


def test_equal_rows_under_method_5_match_method_3(engine, model):
    """Three rows of 9600 samples (seeds 200, 201, 202: no near-tied frame on the padded input either, margins
    >= 8.4e-4 and >= 1.0e-3 from the threshold at K gap <= 8.6e-5) run as one equal-length batched FCPE pass under
    f0_method 5: every row at the bars above against f0_method 3 on that row alone."""
    check_rows_vs_single(engine, [clip(EQUAL_N, s) for s in EQUAL_SEEDS], [0, 3, 7], seed=5, **SHORT_PAD)


def test_workspace_bytes_with_f0_method_5_holds_the_call(engine, model):
    t = engine.torch
    engine.set_pipeline_highpass()
    audios = pipe_clips()
    opts = engine.pipeline_opts(pitch=2.0, protect=0.33, f0_method=5, fcpe_threshold=THR, **SHORT_PAD)
    free = [engine.host(y) for y in engine.pipeline_batch_v(audios, opts, sids=PIPE_SIDS, seed=11)]
    need = engine.workspace_bytes(max(PIPE_NS), len(PIPE_NS), opts)
    o0 = engine.pipeline_opts(pitch=2.0, protect=0.33, **SHORT_PAD)
    assert need >= engine.workspace_bytes(max(PIPE_NS), len(PIPE_NS), o0) > 0  # covers the call under f0_method 0
    arena = t.empty(need, dtype=t.uint8, device=engine.device)
    engine.set_workspace(arena)
    try:
        arena.fill_(0xFF)
        held = [engine.host(y) for y in engine.pipeline_batch_v(audios, opts, sids=PIPE_SIDS, seed=11)]
    finally:
        engine.set_workspace(None)
    assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(held, free))
    engine.check_device_status()


def test_convert_many_with_ragged_fcpe(synth_w, hubert_w, rmvpe_w, model):
    """The clips in shuffled order through RVCX.convert_many(f0_method="fcpe", ragged_f0=True): the results come back
    in input order, each at the waveform bars above against the single-utterance conversion with the same injected
    noise; "crepe" with ragged_f0 is still a ValueError."""
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer import RVCX, Config

    perm = [2, 0, 3, 1]
    clips = [pipe_clips()[i] for i in perm]
    cfg = Config()
    cfg.x_pad = 0.3  # SHORT_PAD
    rvc = RVCX(config=cfg, synth_state=synth_w, synth_cfg=SYNTH_48K_V2, hubert_state=hubert_w, rmvpe_state=rmvpe_w,
               fcpe_weights=(model["raw"], model["cfg"]), fcpe_threshold=THR)
    try:
        upp = rvc.engine.upp

        def noise_fn(i, T):
            r = np.random.default_rng(1000 + i)
            return r.standard_normal((192, T)).astype(np.float32), r.standard_normal(T * upp).astype(np.float32)

        with pytest.raises(ValueError):
            rvc.convert_many(clips, f0_method="crepe", ragged_f0=True)
        outs = rvc.convert_many(clips, pitch=2, f0_method="fcpe", protect=0.33, sid=3, batch=4, max_pad=0.6,
                                noise_fn=noise_fn, ragged_f0=True)
        assert len(outs) == len(clips)
        failed = []
        for i, c in enumerate(clips):
            ez, es = noise_fn(i, (outs[i].shape[0] + 2 * rvc.pipeline.t_pad_tgt) // upp)
            y1 = rvc.pipeline.pipeline(rvc.hubert_model, rvc.net_g, 3, c, 2, "fcpe", None, 0.0, True, 1.0, "v2", 0.33,
                                       eps_z=ez.reshape(-1), eps_src=es)
            assert outs[i].dtype == np.float32
            failed += compare_row(f"clip {i} n={len(c)}", outs[i], y1)  # convert_many returns the waveforms alone
        rvc.engine.check_device_status()
        assert not failed, "; ".join(failed)
    finally:
        rvc.close()
