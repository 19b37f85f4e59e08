"""RMVPE over a batch of rows of different lengths in one pass (rvcx_rmvpe_batch_v), against the oracle in float64 and
against the single-row call, and the ragged pipeline with it (rvcx_pipeline_opts.f0_method 4).

The batch: n = 2720, 4960, 5280, 10080, 16000 samples (synthetic.speech_like, seeds 70..74), the sizes
tests/test_gpu_module_fp64.py anchors:

      n      F    Fp
    2720    18    32
    4960    32    32
    5280    34    64
   10080    64    64
   16000   101   128

Two pairs share a padded frame count but differ in reflect pad (14 / 0 and 30 / 0), one row sits at Fp_max, and the
U-Net's deepest level has heights 1, 1, 2, 2, 4. The batch runs in the given order and reversed.

Against float64 every row is held to rmvpe_parity.check_salience: the salience within K = 8 gaps (absolute)
of anchor(parity_anchor.rmvpe_fn) on that row alone, the decode decisions through rmvpe_parity.check_rmvpe. That
comparison exempts near-tied frames, so it says something only while few frames are near-tied: at most 10 % of any
row's frames may be, at the worst admissible error K gap. On the CPU the oracle gives 1/18, 0/32, 0/34, 3/64 and 1/101
near-tied frames (gaps 2.3e-5 .. 4.1e-5); the test asserts the condition on the margins it computed.

No test sets RVCX_GRU_SPIN_LIMIT; every test ends with a clean device status.
"""
import ctypes

import numpy as np
import pytest

import parity_anchor as pa
import ragged_rows
from parity_anchor import K, anchor, check
from ragged_rows import PIPE_NS, PIPE_SIDS, SHORT_PAD, cents_apart, clip, compare_row, speech
from rmvpe_parity import check_salience, margins

pytestmark = pytest.mark.gpu

NS = (2720, 4960, 5280, 10080, 16000)
FS = (18, 32, 34, 64, 101)


@pytest.fixture(scope="module")
def rows(rmvpe_w):
    """Per row: the audio, the oracle's float64 salience, the fp32-vs-fp64 gap and the frames that are near-tied at
    the worst admissible error K gap (computed once for all tests, never modified)."""
    out = []
    for b, n in enumerate(NS):
        audio = speech(n, seed=70 + b)
        ref, gap = anchor(pa.rmvpe_fn(rmvpe_w, audio[None]))["out"]
        assert ref.shape == (1, FS[b], 360)
        m = margins(ref[0])
        e = K * max(gap, pa.ULP32)
        near = (np.asarray(m["sal_margin"]) <= 2 * e + 1e-7) | (np.abs(np.asarray(m["sal_thr_margin"])) <= e + 1e-7)
        assert near.sum() <= 0.1 * FS[b], f"n={n}: {int(near.sum())} of {FS[b]} frames near-tied at K gap = {e:.2e}"
        ref.setflags(write=False)
        out.append((audio, ref[0], gap, near))
    return out


@pytest.fixture(scope="module")
def single(engine, rows):
    """engine.rmvpe on every row alone: (f0, salience)."""
    return [tuple(engine.host(x) for x in engine.rmvpe(a, 0.03, want_hidden=True)) for a, _, _, _ in rows]


@pytest.mark.parametrize("order", ["given", "reversed"])
def test_ragged_rmvpe_vs_fp64_and_single(engine, rows, single, order):
    """Every row against float64 (check_salience), and against engine.rmvpe on that row alone: F_out and the shapes, the
    same voicing and f0 within 0.1 cent on every frame that is not near-tied (the bound derived in
    check_rows_vs_single's docstring below: two fp32 evaluations of one salience)."""
    idx = list(range(len(NS))) if order == "given" else list(reversed(range(len(NS))))
    f0s, hids = engine.rmvpe_batch_v([rows[i][0] for i in idx], 0.03, want_hidden=True)
    assert len(f0s) == len(hids) == len(idx)
    failed = []
    for f0, hid, i in zip(f0s, hids, idx):
        _, ref, gap, near = rows[i]
        f0, hid = engine.host(f0), engine.host(hid)
        assert f0.shape == (FS[i],) and hid.shape == (FS[i], 360), (NS[i], f0.shape, hid.shape)
        try:
            err = check(f"rmvpe_batch_v {order} row n={NS[i]} vs fp64", hid, ref, gap, K, absolute=True)
            print(f"rmvpe_batch_v {order} row n={NS[i]}: err / gap {err / max(gap, pa.ULP32):.3f}")
            check_salience(f"rmvpe_batch_v {order} row n={NS[i]}", f0, hid, ref, gap)
            f1 = single[i][0]
            ok = ~near
            assert np.array_equal(f0[ok] > 0, f1[ok] > 0), "voicing differs from the single run's"
            c = cents_apart(f0[ok], f1[ok])
            print(f"rmvpe_batch_v {order} row n={NS[i]} vs single: {c:.5f} cent")
            assert c <= 0.1, f"f0 {c:.4f} cent from the single run's"
        except AssertionError as e:
            failed.append(f"n={NS[i]}: {e}")
    engine.check_device_status()
    assert not failed, "; ".join(failed)


def test_equal_lengths_give_rmvpe_batch_bits(engine):
    audio = np.stack([speech(5280, seed=80 + b) for b in range(3)])
    f_eq, h_eq = (engine.host(x) for x in engine.rmvpe_batch(audio, 0.03, want_hidden=True))
    f0s, hids = engine.rmvpe_batch_v(list(audio), 0.03, want_hidden=True)
    for b in range(3):
        assert np.array_equal(engine.host(f0s[b]), f_eq[b]) and np.array_equal(engine.host(hids[b]), h_eq[b])
    one = engine.rmvpe_batch_v([audio[1]])
    assert np.array_equal(engine.host(one[0]), engine.host(engine.rmvpe(audio[1])))


def run_rows(engine, audios):
    f0s, hids = engine.rmvpe_batch_v(audios, 0.03, want_hidden=True)
    return [engine.host(x) for x in f0s + hids]


def run_rows_c(engine, audios, fill=0.0, lda=None, ldf=None, ld_hidden=None):
    """rvcx_rmvpe_batch_v itself on a batch buffer this test stages: `fill` past every row's end, rows lda samples
    apart, f0 rows ldf and salience rows ld_hidden frames apart (default: the longest row's own). The f0 and salience
    buffers start as NaN. Returns what run_rows returns."""
    t = engine.torch
    ns = [len(a) for a in audios]
    B, lda = len(ns), max(ns) if lda is None else lda
    F = 1 + max(ns) // 160
    ldf, ld_hidden = F if ldf is None else ldf, F if ld_hidden is None else ld_hidden
    a = t.full((B, lda), float(fill), dtype=t.float32, device=engine.device)
    for b, r in enumerate(audios):
        a[b, : ns[b]] = t.as_tensor(r, dtype=t.float32)
    f0 = t.full((B, ldf), float("nan"), dtype=t.float64, device=engine.device)
    hid = t.full((B, ld_hidden, 360), float("nan"), dtype=t.float32, device=engine.device)
    F_arr = (ctypes.c_int64 * B)()
    engine._check(engine.lib.rvcx_rmvpe_batch_v(engine.ctx, a.data_ptr(), (ctypes.c_int64 * B)(*ns), lda, B, 0.03,
                                                f0.data_ptr(), ldf, F_arr, hid.data_ptr(), ld_hidden, engine.stream()),
                  "rmvpe_batch_v")
    assert [int(v) for v in F_arr] == [1 + n // 160 for n in ns]
    return [engine.host(f0[b, : F_arr[b]]) for b in range(B)] + [engine.host(hid[b, : F_arr[b]]) for b in range(B)]


def test_deterministic_and_stale_scratch_does_not_reach_a_row(engine, rows):
    """The call twice gives the same bits. With an attached arena full of NaN bit patterns and then of zeros, every
    row's f0 and salience are finite and the same bits again: nothing past a row's end (another row's frames, the pad
    frames of its own image, scratch no kernel wrote) reaches it."""
    t = engine.torch
    audios = [rows[i][0] for i in (2, 4, 0, 3, 1)]
    first, second = run_rows(engine, audios), run_rows(engine, audios)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    arena = t.empty(256 << 20, dtype=t.uint8, device=engine.device)  # the U-Net's activations at B = 5, 128 frames: ~70 MB
    engine.set_workspace(arena)
    try:
        outs = []
        for fill in (0xFF, 0x00):
            arena.fill_(fill)
            outs.append(run_rows(engine, audios))
    finally:
        engine.set_workspace(None)
    for a, b, c in zip(first, *outs):
        assert np.isfinite(b).all() and np.array_equal(b, c) and np.array_equal(a, b)


def test_audio_past_a_row_end_is_never_read(engine, rows):
    audios = [rows[i][0] for i in (0, 4, 2)]
    clean = run_rows(engine, audios)
    dirty = run_rows_c(engine, audios, fill=float("nan"))
    assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(clean, dirty))
    engine.check_device_status()


@pytest.mark.parametrize("equal", [False, True])
def test_row_strides_wider_than_the_rows(engine, rows, equal):
    """Audio rows, f0 rows and salience rows further apart than the longest row needs (lda, ldf, ld_hidden_frames):
    the same bits as the tight layout. With equal lengths this is the equal-length pass's strided copy-out."""
    audios = [speech(5280, seed=80 + b) for b in range(3)] if equal else [rows[i][0] for i in (1, 4, 2)]
    tight = run_rows(engine, audios)
    F = 1 + max(len(a) for a in audios) // 160
    wide = run_rows_c(engine, audios, lda=max(len(a) for a in audios) + 37, ldf=F + 5, ld_hidden=F + 3)
    assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(tight, wide))
    engine.check_device_status()


def call_v(engine, ns, lda, B, ldf, a=None):
    """rvcx_rmvpe_batch_v itself on a zero buffer of B x lda samples (or `a`)."""
    t = engine.torch
    a = t.zeros((max(B, 1), lda), dtype=t.float32, device=engine.device) if a is None else a
    f0 = t.empty((max(B, 1), max(ldf, 1)), dtype=t.float64, device=engine.device)
    n_arr = (ctypes.c_int64 * max(B, 1))(*ns)
    engine._check(engine.lib.rvcx_rmvpe_batch_v(engine.ctx, a.data_ptr(), n_arr, lda, B, 0.03, f0.data_ptr(), ldf, None,
                                                None, 0, engine.stream()), "rmvpe_batch_v")


def test_refusals(engine):
    from rvcx._lib import RvcxError

    with pytest.raises(RvcxError) as e:  # a row rvcx_rmvpe refuses, with its status
        engine.rmvpe_batch_v([speech(5000, 1), speech(512, 2)])
    assert e.value.code == -2
    with pytest.raises(RvcxError) as e:
        engine.rmvpe(speech(512, 2))
    assert e.value.code == -2
    with pytest.raises(RvcxError) as e:  # no rows
        call_v(engine, [5000], 5000, 0, 64)
    assert e.value.code == -1
    with pytest.raises(RvcxError) as e:  # f0 rows too short for the longest row's 57 frames
        call_v(engine, [5000, 9000], 9000, 2, 40)
    assert e.value.code == -6
    # a row of more than 32000 padded frames (320 s), which only the single-row call chunks: refused on the host, before
    # anything is launched (the 41 MB of zeros are never read)
    n_long = 32001 * 160
    with pytest.raises(RvcxError) as e:
        call_v(engine, [n_long, 16000], n_long, 2, 1 + n_long // 160)
    assert e.value.code == -2 and "32000" in str(e.value)
    engine.check_device_status()


# ----------------------------------------------------------------- the ragged pipeline with f0_method 4
# the rows and the 0.3 s pad of ragged_rows (PIPE_NS, SHORT_PAD: t_pad_tgt = 30 frames, three times the generator's field)
PIPE_SEEDS = (112, 218, 334, 502)


def pipe_clips():
    return [clip(n, s) for n, s in zip(PIPE_NS, PIPE_SEEDS)]


def check_rows_vs_single(engine, audios, sids, seed, **kw):
    """tests/test_gpu_ragged_batch.py's procedure with the rows' f0 from one ragged RMVPE pass (f0_method 4): every row
    against pipeline_ex (f0_method 0) on that utterance alone with its slice of the noise: equal shape and n_out,
    spectrogram correlation > 0.999, max difference < 5e-3 of the peak, and the adjusted f0 with the same voicing and
    within 0.1 cent on EVERY frame. The ragged pass sums in another order than the single-row one (as rvcx_rmvpe_batch
    against rvcx_rmvpe), so its f0 is not the single run's bit for bit; 0.1 cent is the roundoff of the decode, not a
    bar fitted to the result: f0 is 10 * 2^(c / 1200) with c the salience-weighted mean of nine 20-cent bins, so two
    fp32 evaluations of the salience, each within the 5e-5 (absolute) fp32-vs-float64 gap of DESIGN.md section 5 on
    weights that sum to at least the 0.03 threshold, move c by at most 2 * 5e-5 * (sum of |bin - mean| <= 400 cents) /
    0.03 = 1.3 cents in the worst case and by about 0.01 cent at typical weight sums near 1; 0.1 cent lies between and
    is 500 times tighter than the 50 cents of the oracle tests. No frame is exempt, so the clips are chosen (on the
    CPU, from the float64 oracle's salience of each row's high-passed, reflect-padded input) to have no frame whose
    argmax or voicing decision is near-tied at K gap: see PIPE_SEEDS."""
    ragged_rows.check_rows_vs_single(engine, audios, sids, seed, dict(f0_method=4), {}, pitch=2.0, protect=0.33, **kw)


@pytest.mark.parametrize("envelope", [1.0, 0.5])
def test_ragged_f0_pipeline_matches_single(engine, envelope):
    """PIPE_NS with PIPE_SEEDS: per row the first seed from 100, 200, 300, 500 on whose input, high-passed and
    reflect-padded by 4800 samples as the pipeline pads it, has no near-tied frame in the float64 oracle's salience: the
    smallest top-1 / top-2 margin over the row's frames exceeds 2 K gap and the top bin's distance from the 0.03
    threshold exceeds K gap (K = 8, gap the oracle's own fp32-vs-fp64 difference on that input). Computed on the CPU:

          n   seed     F      gap     K gap   min margin   min |top - 0.03|
       8000    112   111   1.86e-5   1.49e-4    7.49e-4        0.828
       9600    218   121   4.28e-5   3.43e-4    9.50e-4        0.849
      12000    334   136   5.46e-5   4.37e-4    1.22e-3        0.846
      10400    502   126   3.21e-5   2.56e-4    5.87e-4        0.841
    """
    check_rows_vs_single(engine, pipe_clips(), PIPE_SIDS, seed=3, volume_envelope=envelope, **SHORT_PAD)


def test_workspace_bytes_with_f0_method_4_holds_the_call(engine):
    t = engine.torch
    engine.set_pipeline_highpass()
    audios = pipe_clips()
    opts = engine.pipeline_opts(pitch=2.0, protect=0.33, f0_method=4, **SHORT_PAD)
    free = [engine.host(y) for y in engine.pipeline_batch_v(audios, opts, sids=PIPE_SIDS, seed=11)]
    arena = t.empty(engine.workspace_bytes(max(PIPE_NS), len(PIPE_NS), opts), dtype=t.uint8, device=engine.device)
    engine.set_workspace(arena)
    try:
        arena.fill_(0xFF)
        held = [engine.host(y) for y in engine.pipeline_batch_v(audios, opts, sids=PIPE_SIDS, seed=11)]
    finally:
        engine.set_workspace(None)
    assert all(np.isfinite(a).all() and np.array_equal(a, b) for a, b in zip(held, free))


def test_convert_many_with_ragged_f0(synth_w, hubert_w, rmvpe_w):
    """The clips in shuffled order through RVCX.convert_many(ragged_f0=True): the results come back in input order, each
    at the waveform bars above against the single-utterance conversion with the same injected noise; another f0 method
    with ragged_f0 is a ValueError."""
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer import RVCX, Config

    perm = [2, 0, 3, 1]
    clips = [pipe_clips()[i] for i in perm]
    cfg = Config()
    cfg.x_pad = 0.3  # SHORT_PAD
    rvc = RVCX(config=cfg, synth_state=synth_w, synth_cfg=SYNTH_48K_V2, hubert_state=hubert_w, rmvpe_state=rmvpe_w)
    try:
        upp = rvc.engine.upp

        def noise_fn(i, T):
            r = np.random.default_rng(1000 + i)
            return r.standard_normal((192, T)).astype(np.float32), r.standard_normal(T * upp).astype(np.float32)

        with pytest.raises(ValueError):
            rvc.convert_many(clips, f0_method="crepe", ragged_f0=True)
        outs = rvc.convert_many(clips, pitch=2, protect=0.33, sid=3, batch=4, max_pad=0.6, noise_fn=noise_fn,
                                ragged_f0=True)
        assert len(outs) == len(clips)
        failed = []
        for i, c in enumerate(clips):
            ez, es = noise_fn(i, (outs[i].shape[0] + 2 * rvc.pipeline.t_pad_tgt) // upp)
            y1 = rvc.pipeline.pipeline(rvc.hubert_model, rvc.net_g, 3, c, 2, "rmvpe", None, 0.0, True, 1.0, "v2", 0.33,
                                       eps_z=ez.reshape(-1), eps_src=es)
            assert outs[i].dtype == np.float32
            failed += compare_row(f"clip {i} n={len(c)}", outs[i], y1)  # convert_many returns the waveforms alone
        rvc.engine.check_device_status()
        assert not failed, "; ".join(failed)
    finally:
        rvc.close()
