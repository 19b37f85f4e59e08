"""The three kernels of csrc/refinegan.hip at kernel level against float64 (rvcx_rg_resample_dw, rvcx_rg_lerp_up_cat,
rvcx_rg_adain, include/rvcx_test.h). Each reference is plain torch in float64 on the same float32 inputs and each bar
an a-priori fp32 rounding bound (tests/refinegan_ref.py: derived there, not tuned); every case prints its measured
err / bound, which a correct kernel keeps well under 1. tests/test_refinegan_cpu.py shows the bounds refuse a dropped
edge tap, a wrong clamp, align_corners, a wrong half-pixel offset and a transposed noise read.

    resample_dw   random unit taps (the Kaiser kernel's own edge taps are ~1e-6 of its centre and would hide a dropped
                  one) at (orig, width) = (2, 3), (3, 5), (12, 40), and the decoder's real taps for r in {2, 8, 10, 12};
                  T_in in {1, orig - 1, width, K, 3 K + 5}: at the short ones the taps outnumber the input and both
                  clamps (k0, k1) cut; B = 2, C in {16, 48}; guard elements around y
    lerp_up_cat   rate in {2, 8, 10, 12}, T in {1, 2, 37}, C = 32 read from 32- and 64-wide rows, Cd in {16, 8}; the skip
                  columns bit-equal; torch's own float32 F.interpolate reported beside, not asserted
    adain         (B, T, C) = (2, 37, 32), (2, 5, 256) (T != C: a transposed noise read cannot pass), the three modes;
                  the seeded draw itself (x = 0, w = 1, slope 1) on (2, 4096, 32): moments, repeatability, independence

The grid-stride second pass of the three kernels starts beyond 2.7e8 elements and is not reached here.
"""
import numpy as np
import pytest
import torch

import refinegan_ref as rr

pytestmark = pytest.mark.gpu

GUARD = 301  # sentinel elements before and after the output view


def _rng(*key):
    """PCG64 seeded by the case's own integers."""
    return np.random.Generator(np.random.PCG64(sum(int(k) * p for k, p in zip(key, (7919, 104729, 1299709, 15485863)))))


def _guarded(engine, shape):
    """A float32 device buffer of sentinels with a contiguous view of `shape` GUARD elements in."""
    n = int(np.prod(shape))
    buf = torch.from_numpy(np.full(n + 2 * GUARD, rr.SENTINEL, np.float32)).to(engine.device)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    h = buf.cpu().numpy().view(np.uint32)
    s = rr.SENTINEL.view(np.uint32)
    return bool((h[:GUARD] == s).all() and (h[-GUARD:] == s).all())


def _resample_cases():
    out = []
    for orig, width in rr.UNIT_TAPS:
        for T in rr.resample_lengths(orig, width):
            for C in (16, 48):
                out.append(pytest.param("unit", orig, width, T, C, id=f"unit-o{orig}w{width}-T{T}-C{C}"))
    for r in rr.RATES:
        _, width = rr.real_taps(r)
        for T in rr.resample_lengths(r, width):
            out.append(pytest.param("real", r, width, T, 16 if T > 1000 else 48, id=f"kaiser-r{r}-T{T}"))
    return out


@pytest.mark.parametrize("taps,orig,width,T,C", _resample_cases())
def test_resample_dw_vs_fp64(engine, taps, orig, width, T, C):
    B, K = 2, 2 * width + orig
    rng = _rng(orig, width, T, C)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    if taps == "unit":
        ker = rng.standard_normal(K).astype(np.float32)
        ker[[0, -1]] = np.where(np.abs(ker[[0, -1]]) < 0.5, 1.0, ker[[0, -1]])  # edge taps of unit size
    else:
        ker, w2 = rr.real_taps(orig)
        assert w2 == width
    ref, bound = rr.resample_ref(x, ker, orig, width)
    T_out = -(-T // orig)
    assert ref.shape == (B, T_out, C)
    buf, y = _guarded(engine, (B, T_out, C))
    up = lambda a: torch.from_numpy(a).to(engine.device)  # noqa: E731
    engine.rg_resample_dw(up(x), up(ker), orig, width, y)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    q = rr.ratio(got, ref, bound)
    print(f"\nresample_dw {taps} orig {orig} width {width} K {K} T_in {T} C {C}: err/bound {q:.3f}")
    assert q <= 1.0, q
    assert _guards_intact(buf), "resample_dw wrote outside y"


@pytest.mark.parametrize("Cd", [16, 8])
@pytest.mark.parametrize("ldx", [32, 64])
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("rate", rr.RATES)
def test_lerp_up_cat_vs_fp64(engine, rate, T, ldx, Cd):
    B, C = 2, 32
    rng = _rng(rate, T, ldx, Cd)
    xw = rng.standard_normal((B, T, ldx)).astype(np.float32)
    xw[..., C:] = np.nan  # the columns of a wider buffer the kernel must not read
    skip = rng.standard_normal((B, T * rate, Cd)).astype(np.float32)
    ref, bound = rr.lerp_ref(xw[..., :C], skip, rate)
    buf, y = _guarded(engine, (B, T * rate, C + Cd))
    up = lambda a: torch.from_numpy(a).to(engine.device)  # noqa: E731
    engine.rg_lerp_up_cat(up(xw), C, rate, 0.2, up(skip), y)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got).all(), "a column beyond C was read"
    q = rr.ratio(got[..., :C], ref[..., :C], bound)
    assert np.array_equal(got[..., C:].view(np.uint32), skip.view(np.uint32)), "skip columns are not copies"
    t32 = torch.nn.functional.interpolate(
        torch.nn.functional.leaky_relu(torch.from_numpy(xw[..., :C]), 0.2).permute(0, 2, 1), scale_factor=float(rate),
        mode="linear").permute(0, 2, 1).numpy()
    diff = np.abs(got[..., :C].astype(np.float64) - t32)
    print(f"\nlerp_up_cat rate {rate} T {T} ldx {ldx} Cd {Cd}: err/bound {q:.3f}; vs torch float32 interpolate: "
          f"{int((diff > 0).sum())} of {diff.size} elements differ, max {float(diff.max()):.2e}")
    assert q <= 1.0, q
    assert _guards_intact(buf), "lerp_up_cat wrote outside y"


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["store", "add", "add_div3"])
@pytest.mark.parametrize("shape", [(2, 37, 32), (2, 5, 256)], ids=["2x37x32", "2x5x256"])
def test_adain_vs_fp64(engine, shape, mode):
    B, T, C = shape
    rng = _rng(B, T, C, mode)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    w = rng.standard_normal(C).astype(np.float32)
    eps = rng.standard_normal((B, C, T)).astype(np.float32)
    y0 = rng.standard_normal((B, T, C)).astype(np.float32)
    ref, bound = rr.adain_ref(x, w, eps, y0, mode, 3.0)
    up = lambda a: torch.from_numpy(a).to(engine.device)  # noqa: E731
    buf, y = _guarded(engine, (B, T, C))
    y.copy_(up(y0) if mode else torch.full((B, T, C), float("nan"), device=engine.device))
    engine.rg_adain(up(x), up(w), up(eps), y, slope=0.2, mode=mode, div=3.0)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert np.isfinite(got).all()
    q = rr.ratio(got, ref, bound)
    print(f"\nadain {shape} mode {mode}: err/bound {q:.3f}")
    assert q <= 1.0, q
    assert _guards_intact(buf), "adain wrote outside y"


def test_adain_seeded_draw(engine):
    """eps = NULL: the kernel draws N(0, 1) from Philox(seed) at the noise's own index. With x = 0, w = 1, slope 1 the
    output is the draw: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n) (five standard errors of n independent
    normals), the same seed repeats bit for bit, two seeds share no run of 8 equal values, everything finite."""
    B, T, C = 2, 4096, 32
    n = B * T * C
    x = torch.zeros((B, T, C), device=engine.device)
    w = torch.ones((C,), device=engine.device)

    def draw(seed):
        y = torch.full((B, T, C), float("nan"), device=engine.device)
        engine.rg_adain(x, w, None, y, slope=1.0, mode=0, seed=seed)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    a, a2, b = draw(5), draw(5), draw(6)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    mean, var = float(a.astype(np.float64).mean()), float(a.astype(np.float64).var())
    print(f"\nadain seeded draw n {n}: mean {mean:+.2e} (bound {5 / np.sqrt(n):.2e}), var - 1 {var - 1:+.2e} "
          f"(bound {5 * np.sqrt(2 / n):.2e})")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert not rr.shares_run(a, b, 8)
    assert rr.shares_run(a, a2, 8)  # the probe finds a run where there is one


def test_entries_refuse_bad_extents(engine):
    """RVCX_E_INVALID (-1) for a null pointer or a count below 1, RVCX_E_SHAPE (-2) for a geometry the kernels do not
    serve; nothing is launched (y keeps its sentinel)."""
    e, dev = engine, engine.device
    buf, y = _guarded(e, (2, 4, 8))
    x = torch.zeros((2, 4, 8), device=dev)
    k = torch.zeros((8,), device=dev)
    s = e.stream()
    rc = e.lib.rvcx_rg_resample_dw
    assert rc(e.ctx, None, 2, 4, 8, k.data_ptr(), 2, 3, y.data_ptr(), 2, s) == -1
    assert rc(e.ctx, x.data_ptr(), 2, 0, 8, k.data_ptr(), 2, 3, y.data_ptr(), 2, s) == -1
    assert rc(e.ctx, x.data_ptr(), 2, 4, 8, k.data_ptr(), 2, 3, y.data_ptr(), 3, s) == -2  # T_out > ceil(4 / 2)
    assert rc(e.ctx, x.data_ptr(), 2, 4, 8, k.data_ptr(), 2, 4096, y.data_ptr(), 2, s) == -2  # 8194 taps
    lc = e.lib.rvcx_rg_lerp_up_cat
    assert lc(e.ctx, x.data_ptr(), 2, 4, 8, 8, 0, 0.2, x.data_ptr(), 4, y.data_ptr(), 12, s) == -1
    assert lc(e.ctx, x.data_ptr(), 2, 4, 8, 7, 2, 0.2, x.data_ptr(), 4, y.data_ptr(), 12, s) == -2  # ldx < C
    assert lc(e.ctx, x.data_ptr(), 2, 4, 8, 8, 2, 0.2, x.data_ptr(), 4, y.data_ptr(), 11, s) == -2  # ldy < C + Cd
    ad = e.lib.rvcx_rg_adain
    assert ad(e.ctx, x.data_ptr(), 2, 4, 8, None, None, 0, 0.2, y.data_ptr(), 0, 1.0, s) == -1
    assert ad(e.ctx, x.data_ptr(), 2, 4, 8, k.data_ptr(), None, 0, 0.2, y.data_ptr(), 3, 1.0, s) == -1
    assert ad(e.ctx, x.data_ptr(), 2, 4, 8, k.data_ptr(), None, 0, 0.2, y.data_ptr(), 2, 0.0, s) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == rr.SENTINEL.view(np.uint32)).all()
