"""The resampler's host side: output lengths (rvcx_resample_poly_len), rvcx.resample's plan and taps against scipy
through the closed form, the new entries' declarations, and the host loader left as it was. No GPU."""
import ctypes
import os
import re
from math import gcd

import numpy as np
import pytest
from scipy import signal
from scipy.io import wavfile

from resample_ref import CPU_PAIRS, bound, closed_form, parent_load_audio, worst_ratio

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _len(n, up, down):
    from rvcx import _lib

    v = ctypes.c_int64(-1)
    rc = _lib.load().rvcx_resample_poly_len(int(n), int(up), int(down), ctypes.byref(v))
    return rc, int(v.value)


@pytest.mark.parametrize("name,rate_in,rate_out", CPU_PAIRS)
def test_output_length_is_scipys(name, rate_in, rate_out):
    g = gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    for n in (1, 2, down - 1, down, down + 1, 257):
        want = len(signal.resample_poly(np.zeros(n), up, down))
        assert _len(n, up, down) == (0, want), (n, up, down)
        assert _len(n, rate_out, rate_in) == (0, want), "the ratio is reduced by its gcd"
    n = 2 ** 33
    assert _len(n, up, down) == (0, -(-n * up // down))


def test_output_length_rejects_bad_arguments():
    assert _len(-1, 1, 3)[0] == -1
    assert _len(5, 0, 3)[0] == -1
    assert _len(5, 1, -3)[0] == -1
    assert _len(2 ** 62, 441, 1)[0] == -1  # does not fit an int64


@pytest.mark.parametrize("name,rate_in,rate_out", CPU_PAIRS)
def test_plan_and_taps_reproduce_scipy(name, rate_in, rate_out):
    """resample.plan / resample.taps in the closed form (numpy float64) against scipy.signal.resample_poly, within
    2 (K + 1) 2^-53 sum|x h| at every output sample."""
    from rvcx import resample

    rng = np.random.default_rng(5)
    h = resample.taps(rate_out, rate_in)
    worst = 0.0
    for n in (1, 2, 257):
        up, down, n_out, n_pre_pad, n_pre_remove = resample.plan(n, rate_out, rate_in)
        assert (up, down) == (rate_out // gcd(rate_in, rate_out), rate_in // gcd(rate_in, rate_out))
        half = 10 * max(up, down)
        assert len(h) == 2 * half + 1
        assert n_pre_pad == down - half % down and n_pre_remove == (half + n_pre_pad) // down
        x = rng.standard_normal(n)
        ref = signal.resample_poly(x, up, down)
        assert n_out == len(ref)
        y, absum = closed_form(x, h, up, down, n_pre_pad, n_pre_remove, n_out)
        r = worst_ratio(y, ref, bound(absum, len(h), up))
        worst = max(worst, r)
        assert r <= 1.0, (name, n, r)
    print(f"closed form vs scipy {name}: worst |diff| / bound = {worst:.3f}")


def test_taps_are_cached_and_identity_is_one_tap():
    from rvcx import resample

    assert resample.taps(16000, 48000) is resample.taps(1, 3)
    assert not resample.taps(1, 3).flags.writeable
    assert resample.taps(16000, 16000).tolist() == [1.0]
    assert resample.plan(7, 5, 5) == (1, 1, 7, 1, 1)
    with pytest.raises(ValueError):
        resample.plan(7, 0, 5)


def test_entries_are_declared_once_with_one_signature():
    from rvcx import _lib

    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rvcx.h")).read(), flags=re.S)
    for name in ("rvcx_resample_poly_len", "rvcx_resample_poly_v"):
        protos = re.findall(r"^\s*int\s+" + name + r"\s*\(([^;{}]*)\)\s*;", src, re.M)
        assert len(protos) == 1, name
        assert name in _lib.SIG and name not in _lib.TEST_SIG
        assert len(protos[0].split(",")) == len(_lib.SIG[name][1]), name
        assert name in _lib.exported_symbols()
    v = re.search(r"rvcx_resample_poly_v\s*\(([^;{}]*)\)", src).group(1)
    assert [p.split()[-1].lstrip("*") for p in v.split(",")] == [
        "ctx", "d_x", "dtype", "channels", "n", "ldx", "B", "up", "down", "d_taps", "ntaps", "d_y", "ldy", "n_out",
        "stream"]


def test_host_loader_is_unchanged(tmp_path):
    """load_audio(path) without an engine: bit-equal to the loader as it stood, on a 44.1 kHz stereo int16 file."""
    from rvcx.infer.infer import load_audio

    rng = np.random.default_rng(11)
    data = rng.integers(-32768, 32768, size=(4410, 2)).astype(np.int16)
    path = str(tmp_path / "stereo44k1.wav")
    wavfile.write(path, 44100, data)
    got, want = load_audio(path), parent_load_audio(path)
    assert got.dtype == np.float64 and got.shape == want.shape == (1600,)
    assert np.array_equal(got, want)
