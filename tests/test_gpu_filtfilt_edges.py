"""The chunk-parallel cascaded-SOS filtfilt (csrc/iir_scan.hip, through Engine.highpass_pad) at its structural edges,
against scipy.signal.sosfiltfilt(sos, x, padtype="odd", padlen=3 (order + 1)) in float64.

Reference: the section form, the arithmetic the device runs. On the CPU it sits 4e-14 - 6e-14 of the peak from an
80-bit restatement (n = 300 and 8292, with and without a DC offset); filtfilt(b, a), the transfer-function form, sits
2e-8 - 4e-8 away (its own rounding noise), so it is not the reference here.

Bound:  max |dev - ref| <= 1e-10 max(peak |ref|, peak |x|).  A structural bar, not a measurement: 100 times the 1e-12
iir_scan.hip and DESIGN.md state, 300 times below the transfer-function form's noise; a missed or misplaced chunk state
is an error of the order of the state itself. The input's peak is in the scale because a constant input gives an
output near 0. The fp32 output must be the fp64 output rounded.

Geometry (order 5: 3 sections, padlen 18, ne = n + 36 samples in the odd extension; chunks of 128 samples, 64 chunks =
8192 samples per block, k_casc_carry walks the earlier blocks in groups of 256):
    n = 19        the smallest legal input (ne = 55); n = 18 must raise, as scipy does
    92 / 93       one chunk / one chunk + 1 sample
    8156 / 8157   one block / one block + 1 sample
    2097116 / 2097117   256 blocks / 257 blocks (the last block's walk fills one group exactly)
    2105310       258 blocks: the last one's walk enters the second group of 256
    2200000       a three-minute song's order of length (2.2 M doubles, 35 MB of workspace)
Every case prints `filtfilt <case>: err/scale ratio-to-bound`.
"""
import numpy as np
import pytest
from scipy import signal

pytestmark = pytest.mark.gpu

BOUND = 1e-10
NMAX = 2200000
SIZES = [19, 92, 93, 8156, 8157, 2097116, 2097117, 2105310, 2200000]
PADLEN = 18
IMPULSES = {"imp_127": 127 - PADLEN, "imp_128": 128 - PADLEN, "imp_8191": 8191 - PADLEN}


@pytest.fixture(scope="module")
def eng():
    from rvcx.engine import Engine

    e = Engine(0)
    e.set_pipeline_highpass()
    yield e
    e.close()


_SPEECH = []


def speech(n):
    """The first n samples of one 2.2 M-sample speech_like signal (generated once, never modified)."""
    if not _SPEECH:
        from rvcx import synthetic

        s = synthetic.speech_like(NMAX, seed=13)
        s.setflags(write=False)
        _SPEECH.append(s)
    return _SPEECH[0][:n]


def make_input(kind, n):
    if kind == "speech":
        return speech(n).copy()
    if kind == "speech_dc":  # the zi steady state
        return speech(n) + 0.5
    if kind == "const":  # output about 0
        return np.full(n, 0.7)
    x = np.zeros(n)  # a unit impulse on the last sample of a chunk / the first of the next / the last of a block (ne)
    x[IMPULSES[kind]] = 1.0
    return x


def check(eng, name, x, sos, order, t_pad):
    ref = np.pad(signal.sosfiltfilt(sos, x, padtype="odd", padlen=3 * (order + 1)), (t_pad, t_pad), mode="reflect")
    p64, p32 = eng.highpass_pad(x, t_pad)
    got = p64.cpu().numpy()
    eng.check_device_status()
    assert got.shape == ref.shape and np.isfinite(got).all(), name
    scale = max(float(np.abs(ref).max()), float(np.abs(x).max()))
    err = float(np.abs(got - ref).max()) / scale
    print(f"\nfiltfilt {name}: err {err:.3e} of the scale, bound {BOUND:.0e}, ratio {err / BOUND:.2e}")
    assert err <= BOUND, f"filtfilt {name}: {err:.3e} of the scale > {BOUND:.0e}"
    assert np.array_equal(p32.cpu().numpy(), got.astype(np.float32)), name


def cases():
    out = []
    for n in SIZES:
        kinds = ["speech", "speech_dc", "const"] + [k for k, at in IMPULSES.items() if at < n]
        if n > 2000000:  # the long ones: every impulse says the same as the one on the block edge
            kinds = ["speech", "speech_dc", "const", "imp_8191"]
        out += [(n, k) for k in kinds]
    return out


@pytest.mark.parametrize("n,kind", cases())
def test_filtfilt_sizes(eng, n, kind):
    sos = signal.butter(N=5, Wn=48, btype="high", fs=16000, output="sos")
    check(eng, f"n={n} {kind}", make_input(kind, n), sos, 5, min(16000, n - 1))


@pytest.mark.parametrize("n", [93, 8157])
@pytest.mark.parametrize("which", ["0", "1", "n-1"])
def test_filtfilt_reflect_pad(eng, n, which):
    t_pad = {"0": 0, "1": 1, "n-1": n - 1}[which]
    sos = signal.butter(N=5, Wn=48, btype="high", fs=16000, output="sos")
    check(eng, f"n={n} t_pad={t_pad}", make_input("speech_dc", n), sos, 5, t_pad)


@pytest.mark.parametrize("n", [8157, 216100])
@pytest.mark.parametrize("order", [2, 4, 8])
def test_filtfilt_section_counts(eng, order, n):
    """Butterworth high-pass of order 2, 4, 8: 1, 2, 4 sections (casc_filtfilt<1 | 2 | 4>), padlen 9, 15, 27."""
    b, a = signal.butter(N=order, Wn=48, btype="high", fs=16000)
    sos = signal.butter(N=order, Wn=48, btype="high", fs=16000, output="sos")
    assert sos.shape == (order // 2, 6)
    try:
        eng.set_highpass(b, a, signal.lfilter_zi(b, a), sos)
        check(eng, f"order={order} n={n}", make_input("speech_dc", n), sos, order, 160)
    finally:
        eng.set_pipeline_highpass()


def test_filtfilt_too_short_raises(eng):
    """n = padlen: scipy refuses (the input must be longer than padlen), and so does the device."""
    from rvcx import _lib

    sos = signal.butter(N=5, Wn=48, btype="high", fs=16000, output="sos")
    x = make_input("speech", PADLEN)
    with pytest.raises(ValueError):
        signal.sosfiltfilt(sos, x, padtype="odd", padlen=PADLEN)
    with pytest.raises(_lib.RvcxError):
        eng.highpass_pad(x, 0)
    eng.check_device_status()
    check(eng, "n=19 after the refusal", make_input("speech", 19), sos, 5, 0)
