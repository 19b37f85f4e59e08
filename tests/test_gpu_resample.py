"""The device resampler (rvcx_resample_poly_v: decode, downmix and scipy.signal.resample_poly in one launch) and what is
built on it: load_audio(engine=), device_load= and resample_sr= of rvcx.infer.RVCX.

Every comparison with scipy or with the numpy closed form holds at every output sample within the bound derived in
tests/resample_ref.py, 2 (K + 1) 2^-53 sum_i |x[i] h[c - i up]|; each case prints its largest |diff| / bound
(profiles/resample_gpu_tests.txt keeps one run's figures)."""
import ctypes
import os
from math import gcd

import numpy as np
import pytest
from scipy import signal
from scipy.io import wavfile

from resample_ref import GPU_PAIRS, bound, closed_form, worst_ratio

pytestmark = pytest.mark.gpu

DT = {np.dtype("float64"): 0, np.dtype("float32"): 1, np.dtype("int16"): 2, np.dtype("int32"): 3}


def ratio_of(rate_in, rate_out):
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def call(eng, rows, up, down, h, channels=1, ldy=None, poison=True):
    """rvcx_resample_poly_v on host rows of one dtype -> (rc, y [B, ldy] numpy, n_out list). The output buffer is
    filled with NaN first, so what the call leaves unwritten shows."""
    import torch

    B = len(rows)
    ns = [r.size // channels for r in rows]
    ldx = max(ns)
    hx = np.zeros((B, ldx * channels), dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        hx[b, : r.size] = r.reshape(-1)
    x = torch.as_tensor(hx, device=eng.device)
    taps = torch.as_tensor(np.array(h, dtype=np.float64), device=eng.device)
    want = [-(-n * up // down) for n in ns]
    ldy = max(want) if ldy is None else ldy
    y = torch.full((B, max(1, ldy)), float("nan") if poison else 0.0, dtype=torch.float64, device=eng.device)
    no = (ctypes.c_int64 * B)()
    rc = eng.lib.rvcx_resample_poly_v(eng.ctx, x.data_ptr(), DT[rows[0].dtype], channels, (ctypes.c_int64 * B)(*ns),
                                      ldx, B, up, down, taps.data_ptr(), taps.numel(), y.data_ptr(), ldy, no,
                                      eng.stream())
    return rc, eng.host(y), [int(v) for v in no]


def lengths(up, down, L):
    return (1, 2, down, down + 1, 257, 2 * L + 5)


@pytest.mark.parametrize("name,rate_in,rate_out", GPU_PAIRS)
def test_kernel_matches_scipy(engine, name, rate_in, rate_out):
    from rvcx import resample

    up, down = ratio_of(rate_in, rate_out)
    h = resample.taps(up, down)
    rng = np.random.default_rng(17)
    worst = 0.0
    for n in lengths(up, down, len(h)):
        x = rng.standard_normal(n)
        ref = signal.resample_poly(x, up, down)
        _, _, n_out, n_pre_pad, n_pre_remove = resample.plan(n, up, down)
        rc, y, no = call(engine, [x], up, down, h)
        assert rc == 0 and no == [n_out] and n_out == len(ref)
        _, absum = closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out)
        r = worst_ratio(y[0, :n_out], ref, bound(absum, len(h), up))
        worst = max(worst, r)
        assert r <= 1.0, (name, n, r)
    print(f"kernel vs scipy {name} ({up}/{down}): worst |diff| / bound = {worst:.3f}")


# 1/32: the staged window caps a block at fewer outputs than it has threads
@pytest.mark.parametrize("name,rate_in,rate_out", GPU_PAIRS + (("1_32", 32, 1),))
def test_kernel_structure_with_unit_scale_taps(engine, name, rate_in, rate_out):
    """Random unit-scale taps of the filter's length: a dropped or shifted edge tap shows at full scale."""
    from rvcx import resample

    up, down = ratio_of(rate_in, rate_out)
    L = 20 * max(up, down) + 1
    rng = np.random.default_rng(23)
    h = rng.standard_normal(L)
    worst = 0.0
    for n in (1, L // up + 3):
        x = rng.standard_normal(n)
        _, _, n_out, n_pre_pad, n_pre_remove = resample.plan(n, up, down)
        rc, y, no = call(engine, [x], up, down, h)
        assert rc == 0 and no == [n_out]
        ref, absum = closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out)
        r = worst_ratio(y[0, :n_out], ref, bound(absum, L, up))
        worst = max(worst, r)
        assert r <= 1.0, (name, n, r)
    print(f"kernel vs closed form, random taps {name} ({up}/{down}): worst |diff| / bound = {worst:.3f}")


@pytest.mark.parametrize("up,down", [(160, 441), (1, 3)])
def test_ragged_rows_equal_their_own_call(engine, up, down):
    from rvcx import resample

    h = resample.taps(up, down)
    rng = np.random.default_rng(29)
    rows = [rng.standard_normal(n) for n in (1, 257, 2 * len(h) + 5)]
    want = [-(-len(r) * up // down) for r in rows]
    ldy = max(want) + 300  # more than one block of tail
    rc, y, no = call(engine, rows, up, down, h, ldy=ldy)
    assert rc == 0 and no == want
    for b, r in enumerate(rows):
        rc, y1, _ = call(engine, [r], up, down, h)
        assert rc == 0
        assert np.array_equal(y[b, : want[b]], y1[0]), b
        assert np.all(y[b, want[b]:] == 0.0) and y[b].shape == (ldy,)


def host_decode(data):
    """The host loader's arithmetic on what wavfile.read returns."""
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
    data = np.asarray(data, dtype=np.float64)
    return data.mean(axis=1) if data.ndim > 1 else data


def samples(rng, dtype, n, ch):
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        d = rng.integers(info.min, info.max, size=(n, ch), endpoint=True).astype(dtype)
        d[0, 0], d[1, -1] = info.min, info.max
        return d
    return rng.standard_normal((n, ch)).astype(dtype)


@pytest.mark.parametrize("dtype", ["int16", "int32", "float32", "float64"])
@pytest.mark.parametrize("ch", [1, 2])
def test_decode_and_downmix_are_the_host_loaders(engine, dtype, ch):
    d = samples(np.random.default_rng(31), np.dtype(dtype), 300, ch)
    rc, y, no = call(engine, [d], 1, 1, np.ones(1), channels=ch)
    assert rc == 0 and no == [300]
    assert np.array_equal(y[0], host_decode(d if ch > 1 else d[:, 0]))
    got = engine.host(engine.resample_poly(d, 1, 1, channels=ch))
    assert np.array_equal(got, y[0])


def test_six_channels(engine):
    d = samples(np.random.default_rng(37), np.dtype("int16"), 300, 6)
    rc, y, _ = call(engine, [d], 1, 1, np.ones(1), channels=6)
    assert rc == 0
    s = d.astype(np.float64) / 32768.0
    assert np.all(np.abs(y[0] - s.mean(axis=1)) <= 6 * 2.0 ** -53 * np.abs(s).sum(axis=1) / 6)


def test_int16_stereo_resampled(engine):
    from rvcx import resample

    up, down = 160, 441
    h = resample.taps(up, down)
    d = samples(np.random.default_rng(41), np.dtype("int16"), 2000, 2)
    x = host_decode(d)
    ref = signal.resample_poly(x, up, down)
    _, _, n_out, n_pre_pad, n_pre_remove = resample.plan(len(x), up, down)
    rc, y, no = call(engine, [d], up, down, h, channels=2)
    assert rc == 0 and no == [len(ref)]
    _, absum = closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out)
    r = worst_ratio(y[0], ref, bound(absum, len(h), up))
    print(f"int16 stereo 160/441 vs scipy on the host-decoded signal: worst |diff| / bound = {r:.3f}")
    assert r <= 1.0


def write_wav(path, rate, seconds, ch, dtype, seed):
    from rvcx import synthetic

    n = int(round(rate * seconds))
    x = np.stack([synthetic.speech_like(n, seed=seed + c, sr=rate) for c in range(ch)], axis=1)
    if dtype == "int16":
        x = np.round(x * 32767.0).astype(np.int16)
    else:
        x = x.astype(dtype)
    wavfile.write(str(path), rate, x if ch > 1 else x[:, 0])
    return str(path)


@pytest.mark.parametrize("rate,ch,dtype", [(44100, 2, "int16"), (48000, 1, "float32")])
def test_load_audio_on_device_matches_the_host_loader(engine, tmp_path, rate, ch, dtype):
    from rvcx import resample
    from rvcx.infer.infer import load_audio

    path = write_wav(tmp_path / "a.wav", rate, 0.3, ch, dtype, seed=3)
    want = load_audio(path)
    got = load_audio(path, engine=engine)
    assert got.is_cuda and str(got.dtype) == "torch.float64" and tuple(got.shape) == want.shape
    x = host_decode(wavfile.read(path)[1])
    up, down, n_out, n_pre_pad, n_pre_remove = resample.plan(len(x), 16000, rate)
    h = resample.taps(up, down)
    _, absum = closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out)
    r = worst_ratio(engine.host(got), want, bound(absum, len(h), up))
    print(f"load_audio(engine=) vs load_audio, {rate} Hz {ch} ch {dtype}: worst |diff| / bound = {r:.3f}")
    assert r <= 1.0


def test_load_audio_on_device_at_16k_is_exact(engine, tmp_path):
    from rvcx.infer.infer import load_audio

    path = write_wav(tmp_path / "a.wav", 16000, 0.3, 2, "int16", seed=5)
    assert np.array_equal(engine.host(load_audio(path, engine=engine)), load_audio(path))


def test_uint8_wav_takes_the_host_route(engine, tmp_path):
    from rvcx.infer.infer import load_audio

    path = str(tmp_path / "u8.wav")
    wavfile.write(path, 48000, np.random.default_rng(2).integers(0, 256, size=4800).astype(np.uint8))
    assert np.array_equal(engine.host(load_audio(path, engine=engine)), load_audio(path))


# ---------------------------------------------------------------------------------------------- RVCX plumbing
def make_rvc(synth_state, synth_cfg, hubert_w, rmvpe_w):
    from rvcx.infer import RVCX, Config

    cfg = Config()
    cfg.x_pad = 0.2  # the clips are shorter than the default 1 s pad, which the reflect padding refuses
    return RVCX(config=cfg, synth_state=synth_state, synth_cfg=synth_cfg, hubert_state=hubert_w, rmvpe_state=rmvpe_w)


@pytest.fixture(scope="module")
def rvc48(synth_w, hubert_w, rmvpe_w):
    from rvcx.config import SYNTH_48K_V2

    r = make_rvc(synth_w, SYNTH_48K_V2, hubert_w, rmvpe_w)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rvc40(hubert_w, rmvpe_w):
    import synth_configs

    r = make_rvc(synth_configs.weights_for("v2_40k"), synth_configs.CONFIGS["v2_40k"], hubert_w, rmvpe_w)
    yield r
    r.close()


def test_infer_device_load(rvc48, tmp_path):
    from rvcx.infer.infer import load_audio

    path = write_wav(tmp_path / "in.wav", 44100, 0.4, 2, "int16", seed=7)
    eng = rvc48.engine
    out = rvc48.infer(path, str(tmp_path / "dev.wav"), device_load=True)
    want = rvc48.convert(eng.host(load_audio(path, engine=eng)), protect=0.5)
    assert np.array_equal(out, want)
    rate, written = wavfile.read(str(tmp_path / "dev.wav"))
    assert rate == rvc48.tgt_sr and np.array_equal(written, want)
    plain = rvc48.infer(path, str(tmp_path / "host.wav"))
    off = rvc48.infer(path, str(tmp_path / "off.wav"), device_load=False)
    assert np.array_equal(plain, off)
    assert np.array_equal(wavfile.read(str(tmp_path / "host.wav"))[1], wavfile.read(str(tmp_path / "off.wav"))[1])


def test_infer_batch_device_load(rvc48, tmp_path):
    from rvcx.infer.infer import load_audio, load_audio_device

    src = tmp_path / "in"
    src.mkdir()
    write_wav(src / "a.wav", 44100, 0.40, 2, "int16", seed=11)
    write_wav(src / "b.wav", 48000, 0.50, 1, "float32", seed=13)
    write_wav(src / "c.wav", 44100, 0.42, 2, "int16", seed=17)
    files = [str(src / f) for f in ("a.wav", "b.wav", "c.wav")]
    paths = rvc48.infer_batch(str(src), str(tmp_path / "dev"), device_load=True)
    rows = load_audio_device(files, rvc48.engine)
    for f, r in zip(files, rows):  # a grouped row is the file's own load
        assert np.array_equal(rvc48.engine.host(r), rvc48.engine.host(load_audio(f, engine=rvc48.engine)))
    want = rvc48.convert_many(rows)
    assert [os.path.basename(p) for p in paths] == ["a.wav", "b.wav", "c.wav"]
    for p, w in zip(paths, want):
        rate, got = wavfile.read(p)
        assert rate == rvc48.tgt_sr and np.array_equal(got, w)
    plain = rvc48.infer_batch(str(src), str(tmp_path / "host"))
    off = rvc48.infer_batch(str(src), str(tmp_path / "off"), device_load=False)
    for p, q in zip(plain, off):
        assert np.array_equal(wavfile.read(p)[1], wavfile.read(q)[1])


@pytest.mark.parametrize("which", ["48k", "40k"])
def test_resample_sr(request, tmp_path, which):
    """convert(x, resample_sr=44100): the float32 output resampled in fp64 and rounded to float32 once, so within
    bound + 2^-24 |y| of scipy on the float32 output (y the delivered sample: the final rounding is at most half an
    ulp of it)."""
    from rvcx import resample, synthetic

    rvc = request.getfixturevalue("rvc48" if which == "48k" else "rvc40")
    x = synthetic.speech_like(6400, seed=19)
    base = rvc.convert(x)
    for sr in (0, 8000, rvc.tgt_sr):
        assert np.array_equal(rvc.convert(x, resample_sr=sr), base), sr
    got = rvc.convert(x, resample_sr=44100)
    up, down, n_out, n_pre_pad, n_pre_remove = resample.plan(len(base), 44100, rvc.tgt_sr)
    assert got.dtype == np.float32 and got.shape == (n_out,) and n_out == -(-len(base) * up // down)
    x64 = base.astype(np.float64)
    ref = signal.resample_poly(x64, up, down)
    h = resample.taps(up, down)
    _, absum = closed_form(x64, h, up, down, n_pre_pad, n_pre_remove, n_out)
    bnd = bound(absum, len(h), up) + 2.0 ** -24 * np.abs(got.astype(np.float64))
    r = worst_ratio(got, ref, bnd)
    print(f"resample_sr {rvc.tgt_sr} -> 44100 ({up}/{down}): worst |diff| / (bound + 2^-24 |y|) = {r:.3f}")
    assert r <= 1.0
    many = rvc.convert_many([x, x[:5000]], resample_sr=44100, batch=1)
    assert np.array_equal(many[0], got) and many[1].shape == (-(-len(rvc.convert(x[:5000])) * up // down),)
    path = write_wav(tmp_path / "in.wav", 16000, 0.4, 1, "int16", seed=19)
    out = rvc.infer(path, str(tmp_path / "out.wav"), resample_sr=44100)
    rate, written = wavfile.read(str(tmp_path / "out.wav"))
    assert rate == 44100 and np.array_equal(written, out)
    rvc.infer(path, str(tmp_path / "out8.wav"), resample_sr=8000)
    assert wavfile.read(str(tmp_path / "out8.wav"))[0] == rvc.tgt_sr


def test_errors_leave_the_context_usable(engine):
    import torch

    from rvcx import resample

    h = resample.taps(1, 3)
    x = np.random.default_rng(43).standard_normal(100)
    xd = torch.as_tensor(x, device=engine.device)
    hd = torch.as_tensor(np.array(h), device=engine.device)
    yd = torch.zeros(64, dtype=torch.float64, device=engine.device)

    def raw(n, up, down, ntaps, ldy):
        no = (ctypes.c_int64 * 1)()
        return engine.lib.rvcx_resample_poly_v(engine.ctx, xd.data_ptr(), 0, 1, (ctypes.c_int64 * 1)(n), 100, 1, up,
                                               down, hd.data_ptr(), ntaps, yd.data_ptr(), ldy, no, engine.stream())

    assert raw(0, 1, 3, 61, 64) == -1       # RVCX_E_INVALID: an empty row
    assert raw(100, 2, 6, 121, 64) == -2    # RVCX_E_SHAPE: not coprime
    assert raw(100, 0, 3, 61, 64) == -2     # RVCX_E_SHAPE: not positive
    assert raw(100, 1, 3, 59, 64) == -1     # RVCX_E_INVALID: ntaps of another length
    assert raw(100, 1, 3, 61, 33) == -2     # RVCX_E_SHAPE: ldy below ceil(100 / 3) = 34
    assert b"ldy" in engine.lib.rvcx_last_error(engine.ctx)
    assert raw(100, 1, 3, 61, 64) == 0
    got = engine.host(yd)
    ref = signal.resample_poly(x, 1, 3)
    assert np.allclose(got[:34], ref, rtol=0, atol=1e-12) and np.all(got[34:] == 0.0)
