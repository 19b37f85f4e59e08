"""tests/gru_ref.py (the reference of test_gpu_gru.py) pinned to nn.GRU: its unperturbed float64 form against
oracle.rmvpe.bigru in float64 on the same weights, with gi = x W_ih^T + b_ih formed in float64. No GPU."""
import numpy as np
import pytest
import torch

import gru_ref


def _case(B, T, scale, seed):
    rng = np.random.default_rng(seed)
    w = {}
    for sfx in ("", "_reverse"):
        w["fc.0.gru.weight_ih_l0" + sfx] = rng.uniform(-scale, scale, (768, 384))
        w["fc.0.gru.weight_hh_l0" + sfx] = rng.uniform(-scale, scale, (768, 256))
        w["fc.0.gru.bias_ih_l0" + sfx] = rng.uniform(-scale, scale, 768)
        w["fc.0.gru.bias_hh_l0" + sfx] = rng.uniform(-scale, scale, 768)
    x = rng.standard_normal((B, T, 384))
    gi = np.concatenate([x @ w["fc.0.gru.weight_ih_l0" + s].T + w["fc.0.gru.bias_ih_l0" + s] for s in ("", "_reverse")],
                        axis=2)
    return w, x, gi


@pytest.mark.parametrize("B,T,scale", [(1, 1, 1 / 16), (1, 2, 1 / 4), (2, 3, 1 / 4), (1, 33, 1 / 16), (3, 40, 1 / 4)])
def test_gru_ref_matches_nn_gru_fp64(B, T, scale):
    from oracle import rmvpe as orm

    w, x, gi = _case(B, T, scale, seed=7 + T)
    with torch.no_grad():
        ref = orm.bigru(w, torch.from_numpy(x)).numpy()
    got = gru_ref.gru_bidir(gi, w["fc.0.gru.weight_hh_l0"], w["fc.0.gru.bias_hh_l0"],
                            w["fc.0.gru.weight_hh_l0_reverse"], w["fc.0.gru.bias_hh_l0_reverse"], np.float64)
    assert got.shape == ref.shape == (B, T, 512) and got.dtype == np.float64
    err = float(np.abs(got - ref).max())
    print(f"\ngru_ref vs nn.GRU fp64 B={B} T={T} scale={scale}: {err:.2e}")
    assert err <= 1e-12


def _mutant(gi, whh, bhh, kind, at):
    """The forward direction in float64 with one structural slip of the kind the split recurrence can make, at step
    `at`: "stale" -- units 0..127 see the partner half of h (units 128..255) as it was one step earlier (a hand-off
    read from the wrong parity of the double buffer); "frame" -- the input gates of step at - 1; "carry" -- h is not
    carried into the step (a restart from zero)."""
    T = gi.shape[0]
    h = np.zeros(256)
    hist = [h]
    out = np.zeros((T, 256))
    for s in range(T):
        hin = h.copy()
        ig = gi[s]
        if s == at and kind == "carry":
            hin[:] = 0
        if s == at and kind == "frame":
            ig = gi[s - 1]
        hg = whh @ hin + bhh
        if s == at and kind == "stale":
            hs = hin.copy()
            hs[128:] = hist[-2][128:]
            rows = np.concatenate([np.arange(g * 256, g * 256 + 128) for g in range(3)])
            hg[rows] = whh[rows] @ hs + bhh[rows]
        r = 1 / (1 + np.exp(-(hg[:256] + ig[:256])))
        z = 1 / (1 + np.exp(-(hg[256:512] + ig[256:512])))
        n = np.tanh(ig[512:] + hg[512:] * r)
        h = (hin - n) * z + n
        hist.append(h)
        out[s] = h
    return out


@pytest.mark.parametrize("scale", [1 / 16, 1 / 4])
def test_gpu_gru_bound_sees_structural_slips(scale):
    """The bound of tests/test_gpu_gru.py (K max(gap, 2^-23) + E_act, about 3e-6 .. 2e-5) on a case of its kind
    against one slip at one step of a T = 33 run: each lands orders of magnitude beyond it."""
    w, _, gi = _case(1, 33, scale, seed=11)
    a = (w["fc.0.gru.weight_hh_l0"], w["fc.0.gru.bias_hh_l0"], w["fc.0.gru.weight_hh_l0_reverse"],
         w["fc.0.gru.bias_hh_l0_reverse"])
    g32 = gi[0].astype(np.float32)
    a32 = [x.astype(np.float32) for x in a]
    r64 = gru_ref.gru_bidir(g32, *a32)
    gap = np.abs(gru_ref.gru_bidir(g32, *a32, dtype=np.float32) - r64).max()
    e_act = max(np.abs(gru_ref.gru_bidir(g32, *a32, a_s=2e-6, a_t=6e-7, seed=s) - r64).max() for s in (1, 2, 3))
    bound = 8 * max(gap, 2.0 ** -23) + e_act
    assert gap <= 1e-5 and bound < 5e-5, (gap, bound)
    fwd = _mutant(g32[:, :768].astype(np.float64), a32[0].astype(np.float64), a32[1].astype(np.float64), None, -1)
    assert np.abs(fwd - r64[:, :256]).max() <= 1e-12  # the unmutated loop is the reference
    for kind in ("stale", "frame", "carry"):
        for at in (2, 3, 32):  # both parities, and the last step (no later step spreads it)
            m = _mutant(g32[:, :768].astype(np.float64), a32[0].astype(np.float64), a32[1].astype(np.float64), kind, at)
            dev = np.abs(m - r64[:, :256]).max()
            print(f"\nslip {kind} at step {at} scale {scale}: {dev:.2e} = {dev / bound:.0f} x the bound {bound:.2e}")
            assert dev > 100 * bound, (kind, at, dev, bound)


def test_gru_ref_dtype_and_perturbation():
    """The fp32 form runs in fp32; the perturbed form is seeded, differs from the plain one by about its amplitudes
    and leaves the plain one untouched when both amplitudes are 0."""
    w, _, gi = _case(1, 12, 1 / 4, seed=3)
    a = (w["fc.0.gru.weight_hh_l0"], w["fc.0.gru.bias_hh_l0"], w["fc.0.gru.weight_hh_l0_reverse"],
         w["fc.0.gru.bias_hh_l0_reverse"])
    r64 = gru_ref.gru_bidir(gi[0], *a)
    r32 = gru_ref.gru_bidir(gi[0], *a, dtype=np.float32)
    assert r64.shape == (12, 512) and r32.dtype == np.float32
    assert 0 < np.abs(r32 - r64).max() < 1e-5
    p1 = gru_ref.gru_bidir(gi[0], *a, a_s=2e-6, a_t=6e-7, seed=1)
    p1b = gru_ref.gru_bidir(gi[0], *a, a_s=2e-6, a_t=6e-7, seed=1)
    p2 = gru_ref.gru_bidir(gi[0], *a, a_s=2e-6, a_t=6e-7, seed=2)
    assert np.array_equal(p1, p1b) and not np.array_equal(p1, p2)
    d = np.abs(p1 - r64).max()
    assert 1e-8 < d < 1e-4, d
    assert np.array_equal(gru_ref.gru_bidir(gi[0], *a, a_s=0.0, a_t=0.0, seed=5), r64)
