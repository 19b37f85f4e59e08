"""The noise gate's kernels (csrc/spectral_gate.hip through rvcx_spectral_gate) against the torch restatement of
TorchGate's stationary mode in float64 (tests/spectral_gate_ref.py), anchored as tests/parity_anchor.py does it: the
device may stand K = 8 times as far from float64 as torch's own float32 run of the same function on the same input.

The comparison X_db > thresh is discontinuous, so it is held in two parts, row by row:
  mask    gap_m = the anchor's max |margin32 - margin64| (margin = X_db - thresh, dB), delta = 8 gap_m. The device's mask
          must equal margin64 > 0 at every bin with |margin64| > delta, and -- a condition on the inputs, checked on
          the host in test_spectral_gate_cpu.py too -- at most 1 % of a non-silent row's bins may lie inside the band.
  output  y_dev against gate(x, sr, p, float64, mask = the device's mask), the gap from the anchor on that same mask.
Samples [n_out, n) of a gated row must be exactly 0 and nothing beyond n may be written.

Inputs (PCG64(3), t at 48 kHz): row A = 0.3 sin(2 pi 220 t) (sin(2 pi 3 t) > 0) + 0.01 N(0, 1), row B = 0.5 N(0, 1)
linspace(0, 1, n). Shapes: 2048 (9 frames: the 19-tap time filter is wider than the image), 4100 (output 4096, with
row strides above n), 41760 (the streaming hop's row: 164 frames, a tail of 32)."""
import ctypes

import numpy as np
import pytest
import torch

import spectral_gate_ref as ref
from parity_anchor import K, anchor, check

pytestmark = pytest.mark.gpu

RVCX_E_INVALID, RVCX_E_SHAPE = -1, -2
SENTINEL = 12345.0
BAND_SHARE = 0.01

_MARGIN = {}


def _margin(row):
    """(margin64 [513, F], gap_m) of one input row, computed once per row content (it depends on neither sr nor p)."""
    key = row.tobytes()
    if key not in _MARGIN:
        m64, gap = anchor(lambda dt: ref.gate(row[None], 48000, 0.5, dt)[1])["out"]
        _MARGIN[key] = (m64[0], gap)
    return _MARGIN[key]


def _raw(engine, x, sr, strengths, ldx=None, ldy=None, want_mask=True):
    """rvcx_spectral_gate on x [B, n] with the given row strides -> (rc, y [B, ldy] raw, mask [B, 513, F] or None)."""
    t = torch
    B, n = x.shape
    ldx, ldy = ldx or n, ldy or n
    xd = t.full((B, ldx), float("nan"), dtype=t.float32, device=engine.device)
    xd[:, :n] = t.from_numpy(np.ascontiguousarray(x))
    yd = t.full((B, ldy), SENTINEL, dtype=t.float32, device=engine.device)
    md = t.zeros((B, 513, 1 + n // 256), dtype=t.uint8, device=engine.device) if want_mask else None
    st = (ctypes.c_float * B)(*[float(s) for s in np.broadcast_to(strengths, (B,))])
    rc = engine.lib.rvcx_spectral_gate(engine.ctx, xd.data_ptr(), B, n, ldx, int(sr), st, yd.data_ptr(), ldy,
                                       None if md is None else md.data_ptr(), engine.stream())
    t.cuda.synchronize()
    return rc, yd.cpu().numpy(), None if md is None else md.cpu().numpy().astype(bool)


def _hold(engine, x, sr, p, tag, ldx=None, ldy=None):
    """One gated call on x [B, n] held to float64, row by row. Returns the raw device rows."""
    B, n = x.shape
    n_out = ref.n_out(n)
    rc, y, mask = _raw(engine, x, sr, p, ldx, ldy)
    assert rc == 0, (tag, rc)
    assert (y[:, n_out:n] == 0).all(), f"{tag}: samples [n_out, n) are not zero"
    assert (y[:, n:] == SENTINEL).all(), f"{tag}: written beyond n"
    for b in range(B):
        row = np.ascontiguousarray(x[b])
        if not row.any():
            assert not y[b, :n].any(), f"{tag} row {b}: a row of zeros must come back as zeros"
            continue
        m64, gap_m = _margin(row)
        delta = 8 * gap_m
        band = np.abs(m64) <= delta
        share = float(band.mean())
        wrong = int(((mask[b] != (m64 > 0)) & ~band).sum())
        print(f"\n{tag} row {b}: gap_m {gap_m:.3e} dB, {share:.4%} of the bins in the band, "
              f"{int((mask[b] != (m64 > 0)).sum())} flips inside it, {wrong} outside")
        assert share <= BAND_SHARE, (tag, b, share)
        assert wrong == 0, f"{tag} row {b}: {wrong} mask bins differ from float64 outside the band"
        y64, gap = anchor(lambda dt: ref.gate(row[None], sr, p, dt, mask=mask[b][None])[0])["out"]
        check(f"{tag} row {b} y", y[b, :n_out], y64[0], gap, K)
    return y


@pytest.fixture(scope="module")
def rows():
    return {n: ref.gate_rows(n) for n in (2048, 4100, 41760)}


def test_nine_frames(engine, rows):
    _hold(engine, rows[2048], 48000, 0.5, "n2048")


def test_strided_rows_and_small_scale(engine, rows):
    """B = 3 with ldx, ldy > n; the third row is row A scaled by 1e-6 (every threshold is relative to the row)."""
    x = np.concatenate([rows[4100], rows[4100][:1] * np.float32(1e-6)])
    _hold(engine, x, 48000, 0.5, "n4100 strided", ldx=4100 + 28, ldy=4100 + 60)


def test_hop_row(engine, rows):
    """The streaming hop's shape, and the same call twice: the overlap-add has a fixed order."""
    y = _hold(engine, rows[41760], 48000, 0.5, "n41760")
    rc, y2, _ = _raw(engine, rows[41760], 48000, 0.5, want_mask=False)
    assert rc == 0 and np.array_equal(y, y2)
    a = engine.spectral_gate(rows[41760], 48000, 0.5)
    b = engine.spectral_gate(rows[41760], 48000, 0.5)
    assert a.shape == (2, 41728) and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), y[:, :41728])


@pytest.mark.parametrize("sr", [40000, 32000])
def test_other_filter_sizes(engine, rows, sr):
    _hold(engine, rows[4100], sr, 0.5, f"sr{sr}")


@pytest.mark.parametrize("p", [0.0, 1.0])
def test_strength_ends(engine, rows, p):
    _hold(engine, rows[4100], 48000, p, f"p{p}")


def test_zero_row_and_copied_row(engine, rows):
    """[A, zeros, B(copied through), A]: the zero row comes back as zeros, the row with a negative strength bit for bit
    (all n samples), and the two A rows agree with each other and with float64."""
    a, b = rows[4100]
    x = np.stack([a, np.zeros_like(a), b, a])
    strengths = np.array([0.5, 0.5, -1.0, 0.5], np.float32)
    rc, y, mask = _raw(engine, x, 48000, strengths)
    assert rc == 0
    assert not y[1].any()
    assert np.array_equal(y[2], b)
    assert np.array_equal(y[0], y[3]) and np.array_equal(mask[0], mask[3])
    assert not mask[2].any()  # not written for a row that is not gated
    alone = _hold(engine, x[:1], 48000, 0.5, "A alone")
    assert np.array_equal(alone[0], y[0])


def test_refusals(engine, rows):
    rc, y, _ = _raw(engine, rows[2048][:, :2047], 48000, 0.5, want_mask=False)
    assert rc == RVCX_E_SHAPE and (y == SENTINEL).all()
    for sr in (300000, 5000):  # int(500 / (sr / 512)) = 0; int(50 / (256 / sr * 1000)) = 0
        rc, y, _ = _raw(engine, rows[2048], sr, 0.5, want_mask=False)
        assert rc == RVCX_E_SHAPE and (y == SENTINEL).all(), sr
    rc, y, _ = _raw(engine, rows[2048], 48000, 1.5, want_mask=False)
    assert rc == RVCX_E_INVALID and (y == SENTINEL).all()
    with pytest.raises(ValueError):
        engine.spectral_gate(rows[2048], 48000, 1.5)


def test_duck_type(engine, rows):
    from rvcx.infer import SpectralGate

    g = SpectralGate(48000, 0.5, engine=engine)
    y = g(torch.from_numpy(rows[4100]))
    assert y.shape == (2, 4096) and torch.equal(y, engine.spectral_gate(rows[4100], 48000, 0.5))
    with pytest.raises(ValueError):
        SpectralGate(48000, 1.5, engine=engine)
