"""The ragged FCPE pass without a GPU: rvcx_fcpe_batch_v is declared and bound, pipeline_many routes
f0_method="fcpe" with ragged_f0=True to rvcx_pipeline_opts.f0_method 5 (on an engine stub that records the options it
is handed), and the per-row frame bookkeeping of the ragged forward agrees with fcpe_ref.n_frames."""
import types

import numpy as np
import pytest

import fcpe_ref as fr
from abi_headers import header_prototypes

Z = dict(win_size=1024, hop_size=160)  # the front end of every FCPE checkpoint rvc/ ships


def test_entry_point_is_declared_and_bound():
    from rvcx import _lib

    protos = header_prototypes("rvcx.h")
    assert protos.get("rvcx_fcpe_batch_v") == 13
    assert "rvcx_fcpe_batch_v" in _lib.EXPORTS and len(_lib.SIG["rvcx_fcpe_batch_v"][1]) == 13
    # shaped like rvcx_rmvpe_batch_v, plus the decoder mode
    assert len(_lib.SIG["rvcx_rmvpe_batch_v"][1]) == 12
    test = header_prototypes("rvcx_test.h")
    assert test.get("rvcx_performer_attention_v") == 12 == len(_lib.TEST_SIG["rvcx_performer_attention_v"][1])


class _Engine:
    """What pipeline_many touches on an Engine before and at the batched call, recording the options of each call."""

    def __init__(self):
        from rvcx import _lib

        self._lib = _lib
        self.synth_cfg = types.SimpleNamespace(use_f0=True)
        self._hp = True
        self.loaded = {}
        self.upp = 480
        self.calls = []

    def load_fcpe(self, state, config, key=None):
        self.loaded["fcpe"] = key

    def pipeline_opts(self, **kw):
        o = self._lib.PipelineOpts()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def pipeline_batch_v(self, audios, opts, **kw):
        self.calls.append(("batch_v", int(opts.f0_method), [len(a) for a in audios]))
        return [types.SimpleNamespace(cpu=lambda n=len(a): types.SimpleNamespace(numpy=lambda: np.zeros(n, np.float32)))
                for a in audios]

    def pipeline_ex(self, audio, opts, **kw):
        self.calls.append(("ex", int(opts.f0_method), [len(audio)]))
        return np.zeros(len(audio), np.float32)

    def host(self, x):
        return x

    def check_device_status(self):
        pass


def _pipeline(eng, semantics="rvc", fcpe_weights=({"w": np.zeros(1, np.float32)}, {"model": {}})):
    from rvcx.infer import Config, PipelineRVCX

    model = types.SimpleNamespace(engine=eng)
    return PipelineRVCX(48000, Config(), model, None, semantics=semantics, fcpe_weights=fcpe_weights), model


def test_pipeline_many_routes_ragged_fcpe_to_method_5():
    clips = [np.zeros(n) for n in (9000, 9600, 8800)]
    kw = dict(batch=4, max_pad=0.5)
    for method, ragged, want in (("fcpe", True, 5), ("fcpe", False, 3), ("rmvpe", True, 4), ("rmvpe", False, 0)):
        eng = _Engine()
        pl, model = _pipeline(eng)
        outs = pl.pipeline_many(model, None, 0, clips, f0_method=method, ragged_f0=ragged, **kw)
        assert [len(o) for o in outs] == [9000, 9600, 8800]
        assert eng.calls == [("batch_v", want, [9600, 9000, 8800])], (method, ragged, eng.calls)
    # the MLX port's "fcpe" is its RMVPE fallback (method 0): ragged, that is the ragged RMVPE pass
    eng = _Engine()
    pl, model = _pipeline(eng, semantics="mlx")
    pl.pipeline_many(model, None, 0, clips, f0_method="fcpe", ragged_f0=True, **kw)
    assert [c[1] for c in eng.calls] == [4]


def test_pipeline_many_still_refuses_what_it_cannot_run_ragged():
    eng = _Engine()
    pl, model = _pipeline(eng)
    clips = [np.zeros(9000), np.zeros(9600)]
    for method in ("crepe", "crepe-tiny"):
        with pytest.raises(ValueError, match="ragged_f0"):
            pl.pipeline_many(model, None, 0, clips, f0_method=method, ragged_f0=True)
    bare, model = _pipeline(eng, fcpe_weights=None)
    with pytest.raises(ValueError, match="fcpe_weights"):
        bare.pipeline_many(model, None, 0, clips, f0_method="fcpe", ragged_f0=True)
    assert eng.calls == []


# ----------------------------------------------------------------- frame bookkeeping of the ragged forward
def _framing(n, win=1024, hop=160):
    """What fcpe_forward_v computes per row on the host: (zero-padding branch, STFT frames, output frames)."""
    pl = (win - hop) // 2
    pr = max((win - hop + 1) // 2, win - n - pl)
    fs = (n + pl + pr - win) // hop + 1
    nf = n // hop + 1
    return pr >= n, fs, (fs + 1 if nf > fs else nf)


def test_frame_bookkeeping_matches_the_reference():
    """For every length from 1 to 4000 and the test batch's: F_b is fcpe_ref.n_frames; the zero-padding branch is
    exactly n <= 432; and every row outside it has one STFT frame fewer than output frames, so the ragged forward
    repeats each row's own last frame (row F_b - 1 = row F_b - 2) and F_b >= 3 leaves that row in range."""
    for n in list(range(1, 4001)) + [13920, 20480, 48000, 480000]:
        zero, fs, F = _framing(n)
        assert F == fr.n_frames(Z, n) == n // 160 + 1, n
        assert zero == (n <= 432), n
        if not zero:
            assert fs == F - 1 == n // 160 and F >= 3, n
    assert [_framing(n)[2] for n in (1000, 2400, 13920, 20480, 48000)] == [7, 16, 88, 129, 301]
    assert _framing(9000)[2] == 57 and _framing(5000)[2] == 32  # the capacity refusal's 57 frames


def test_mel_rows_of_a_padded_batch():
    """The ragged mel in numpy: STFT frames of a row inside a zero-extended, per-row reflect-padded batch buffer equal
    the frames of that row padded alone, for the rows' own F_b - 1 frames (no frame of a row reads past its own
    padded end), which is what lets the rows share one STFT launch."""
    rng = np.random.default_rng(0)
    ns = (1000, 2400, 700)
    win, hop, pl, pr = 1024, 160, 432, 432
    ld = max(ns) + pl + pr
    buf = np.zeros((len(ns), ld))
    rows = [rng.standard_normal(n) for n in ns]
    for b, x in enumerate(rows):
        buf[b, : len(x) + pl + pr] = np.pad(x, (pl, pr), mode="reflect")
    for b, x in enumerate(rows):
        own = np.pad(x, (pl, pr), mode="reflect")
        fs = _framing(len(x))[1]
        assert (fs - 1) * hop + win <= len(own)
        for f in range(fs):
            assert np.array_equal(buf[b, f * hop: f * hop + win], own[f * hop: f * hop + win])
