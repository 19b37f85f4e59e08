"""RMVPE's BiGRU recurrence at kernel level (csrc/gru.hip k_gru_bidir_g through rvcx_gru_bidir, include/rvcx_test.h)
against tests/gru_ref.py in float64 (pinned to nn.GRU by test_gru_ref_cpu.py). The entry runs the launches RMVPE runs:
the context's hand-off buffer, 16 sequences per launch, one tag counter per 16-sequence slice.

Bound, absolute (|h| <= 1):   err <= K max(gap, 2^-23) + E_act
  * K = 8 and gap = max |gru_ref fp32 - gru_ref fp64| on the case's own inputs: tests/parity_anchor.py's bar for a
    device with other summation orders. Every case asserts gap <= 1e-5, so a chaotic recurrence (weights U(+-1/2):
    fp32 and fp64 part by 2.0 within 300 steps) cannot slip in and make the bound meaningless.
  * E_act covers what the bar above does not: the kernel's activations are the hardware v_exp_f32 / v_rcp_f32 (1 ulp
    each), not correctly rounded ones. It is the largest deviation from float64 of the float64 recurrence with every
    sigmoid perturbed by a relative u a_s and every tanh by an absolute u a_t, u ~ U(-1, 1), over 3 seeds.
      sigm(v) = rcp(1 + exp2(-v log2e)):  the rounding of the scaled argument is |v| log2e 2^-24, i.e. a relative
        0.5 |v| ulp of the exponential; v_exp_f32 adds 1 ulp, the addition 0.5 ulp, v_rcp_f32 1 ulp: (0.5 |v| + 2.5)
        2^-23 relative. A gate saturates (the factor exp / (1 + exp) removes the error) before |v| = 16, where this is
        10.5 ulp = 1.25e-6. a_s = 2e-6.
      tanh_g(v) = 1 - 2 rcp(1 + exp2(2 v log2e)):  near v = 0 the subtracted term is near 1 and carries 0.5 (half of
        the exponential's 1 ulp) + 0.5 (addition) + 1 (rcp) + the argument's share, about 2.5 ulp of 1 = 3.0e-7
        absolute; doubled for the final subtraction's rounding and margin: a_t = 6e-7. (Towards |v| large the term is
        near 0 or near 2 with at most 2 ulp of 1.)
    The amplitudes are derived, not fitted: a case over the bound is a finding.
On the CPU E_act came to 7 - 19 gap, so the bound is about 3e-6 - 2e-5; a wrong index, a stale or missed hand-off or a
wrong carry is an error of the size of h itself, four orders above it.

Every case is a few milliseconds (about 1.2 us per step). No test sets RVCX_GRU_SPIN_LIMIT; every test ends with a
clean device status (no hand-off timed out).
"""
import numpy as np
import pytest

import gru_ref
from parity_anchor import K, ULP32

pytestmark = pytest.mark.gpu

A_S, A_T = 2e-6, 6e-7
H = 256


@pytest.fixture(scope="module")
def eng():
    from rvcx.engine import Engine

    e = Engine(0)
    yield e
    e.close()


def make_case(B, T, gi_sigma, w_scale, seed):
    """fp32 inputs: gi ~ N(0, gi_sigma^2) [B, T, 1536], W_hh / b_hh ~ U(+-w_scale) per direction."""
    rng = np.random.default_rng(seed)
    gi = (gi_sigma * rng.standard_normal((B, T, 6 * H))).astype(np.float32)
    w = [rng.uniform(-w_scale, w_scale, s).astype(np.float32) for s in ((3 * H, H), (3 * H,), (3 * H, H), (3 * H,))]
    return gi, w


_REF = {}


def reference(key, gi, w):
    """(ref64, gap, E_act) of a case, computed once per key and never modified."""
    if key not in _REF:
        r64 = gru_ref.gru_bidir(gi, *w, dtype=np.float64)
        r32 = gru_ref.gru_bidir(gi, *w, dtype=np.float32)
        gap = float(np.abs(r32.astype(np.float64) - r64).max())
        e_act = max(float(np.abs(gru_ref.gru_bidir(gi, *w, dtype=np.float64, a_s=A_S, a_t=A_T, seed=s) - r64).max())
                    for s in (1, 2, 3))
        r64.setflags(write=False)
        _REF[key] = (r64, gap, e_act)
    return _REF[key]


def check_vs_fp64(name, dev, key, gi, w):
    r64, gap, e_act = reference(key, gi, w)
    assert dev.shape == r64.shape and np.isfinite(dev).all(), name
    assert gap <= 1e-5, f"{name}: the case's own fp32-vs-fp64 gap {gap:.2e} is not small: a chaotic recurrence"
    err = float(np.abs(dev.astype(np.float64) - r64).max())
    bound = K * max(gap, ULP32) + e_act
    print(f"\ngru {name}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f} (gap {gap:.2e} E_act {e_act:.2e})")
    assert err <= bound, f"gru {name}: err {err:.3e} > {K} x max(gap {gap:.2e}, 2^-23) + E_act {e_act:.2e} = {bound:.3e}"


def run(eng, gi, w, tag_start=0):
    return eng.gru_bidir(gi, *w, tag_start=tag_start).cpu().numpy()


def done(eng):
    eng.check_device_status()


# ----------------------------------------------------------------- lengths, weight scales, saturating gates
@pytest.mark.parametrize("gi_sigma", [1.0, 4.0])
@pytest.mark.parametrize("w_scale", [1 / 16, 1 / 4])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 32, 33, 300])
def test_gru_vs_fp64(eng, T, w_scale, gi_sigma):
    """T = 1: no hand-off; 2: the first; 3: both parities of the double buffer; 33 and 300 beyond RMVPE's multiples
    of 32. N(0, 4^2) input gates saturate r and z."""
    gi, w = make_case(1, T, gi_sigma, w_scale, seed=1000 + T)
    out = run(eng, gi, w)
    check_vs_fp64(f"T={T} w={w_scale:.4f} gi_sigma={gi_sigma}", out, ("len", T, w_scale, gi_sigma), gi, w)
    done(eng)


# ----------------------------------------------------------------- structural probes
def _probe_weights(w, probe):
    whh_f, bhh_f, whh_b, bhh_b = (x.copy() for x in w)
    for m in (whh_f, whh_b):
        if probe == "whh0":  # closed form per step: checks the gi and reverse-time indexing alone
            m[:] = 0
        elif probe == "own0":  # a unit's own half of h does not reach it: only the partner path acts
            for q in (0, 1):
                for g in range(3):
                    m[g * H + q * 128:g * H + (q + 1) * 128, q * 128:(q + 1) * 128] = 0
        elif probe == "partner0":  # only the workgroup's own half acts
            for q in (0, 1):
                for g in range(3):
                    m[g * H + q * 128:g * H + (q + 1) * 128, (1 - q) * 128:(2 - q) * 128] = 0
        else:  # one gate's rows non-zero at a time
            g = {"gate_r": 0, "gate_z": 1, "gate_n": 2}[probe]
            keep = m[g * H:(g + 1) * H].copy()
            m[:] = 0
            m[g * H:(g + 1) * H] = keep
    return [whh_f, bhh_f, whh_b, bhh_b]


@pytest.mark.parametrize("probe", ["whh0", "own0", "partner0", "gate_r", "gate_z", "gate_n"])
@pytest.mark.parametrize("T", [3, 33])
def test_gru_structural_probes(eng, T, probe):
    gi, w = make_case(1, T, 1.0, 1 / 4, seed=2000 + T)
    w = _probe_weights(w, probe)
    out = run(eng, gi, w)
    check_vs_fp64(f"probe {probe} T={T}", out, ("probe", T, probe), gi, w)
    done(eng)


# ----------------------------------------------------------------- batches: the 16-sequence grouping
@pytest.mark.parametrize("T", [4, 32])
@pytest.mark.parametrize("B", [2, 16, 17, 33])
def test_gru_batch_rows_equal_single_calls(eng, B, T):
    """B > 16 goes out as launches of 16 sequences with one tag counter per slice. Every row against float64, and bit
    for bit the B = 1 call on it: the kernel's summation order is fixed."""
    gi, w = make_case(B, T, 1.0, 1 / 4, seed=3000 + 64 * T + B)
    dw = [eng._dev(x, eng.torch.float32) for x in w]
    out = run(eng, gi, dw)
    check_vs_fp64(f"batch B={B} T={T}", out, ("batch", B, T), gi, w)
    for b in range(B):
        one = run(eng, gi[b:b + 1], dw)
        assert np.array_equal(one[0], out[b]), f"B={B} T={T}: row {b} differs from its B = 1 run"
    done(eng)


# ----------------------------------------------------------------- launches on one buffer, tags running on
def test_gru_launches_continue_tags(eng):
    """T = 5, 2, 7, 1, 3 in a row on one buffer, zeroed before the first only: each output bit-equal to the same
    inputs on a zeroed buffer."""
    cases = [make_case(1, T, 1.0, 1 / 4, seed=4000 + i) for i, T in enumerate((5, 2, 7, 1, 3))]
    chained = [run(eng, gi, w, tag_start=0 if i == 0 else -1) for i, (gi, w) in enumerate(cases)]
    for i, (gi, w) in enumerate(cases):
        fresh = run(eng, gi, w, tag_start=0)
        assert np.array_equal(fresh, chained[i]), f"launch {i} (T={gi.shape[1]}) differs when the tags run on"
        check_vs_fp64(f"chain {i} T={gi.shape[1]}", fresh, ("chain", i), gi, w)
    done(eng)


def test_gru_launches_change_batch(eng):
    """B = 2, then 1, then 2 without asking for a zeroed buffer."""
    cases = [make_case(B, 6, 1.0, 1 / 4, seed=4100 + i) for i, B in enumerate((2, 1, 2))]
    run(eng, *cases[0], tag_start=0)
    chained = [run(eng, gi, w, tag_start=-1) for gi, w in cases]
    for i, (gi, w) in enumerate(cases):
        assert np.array_equal(run(eng, gi, w, tag_start=0), chained[i]), f"launch {i} (B={gi.shape[0]})"
    done(eng)


# ----------------------------------------------------------------- the 32-bit tag space
def test_gru_tag_space_wrap(eng):
    """T = 8. The highest counter that does not wrap (its last tag is 2^32 - 2), then a launch that continues from
    there and wraps (the slice is zeroed and restarts at 1), and a counter that wraps at once: all bit-equal to the
    run on a zeroed buffer."""
    T = 8
    a, b = make_case(1, T, 1.0, 1 / 4, seed=4200), make_case(1, T, 1.0, 1 / 4, seed=4201)
    ref_a, ref_b = run(eng, *a, tag_start=0), run(eng, *b, tag_start=0)
    check_vs_fp64("tags a", ref_a, ("tags", 0), *a)
    check_vs_fp64("tags b", ref_b, ("tags", 1), *b)
    hi = run(eng, *a, tag_start=2 ** 32 - 1 - (T + 1))
    assert np.array_equal(hi, ref_a), "the highest counter that does not wrap"
    wrapped = run(eng, *b, tag_start=-1)
    assert np.array_equal(wrapped, ref_b), "the launch that wraps"
    after = run(eng, *a, tag_start=-1)
    assert np.array_equal(after, ref_a), "the launch after the wrap"
    at_once = run(eng, *b, tag_start=2 ** 32 - 3)
    assert np.array_equal(at_once, ref_b), "a counter that wraps at once"
    done(eng)


def test_gru_bad_arguments(eng):
    from rvcx import _lib

    gi, w = make_case(1, 2, 1.0, 1 / 4, seed=1)
    t = eng.torch
    g = eng._dev(gi, t.float32)
    dw = [eng._dev(x, t.float32) for x in w]
    out = t.empty((1, 2, 512), dtype=t.float32, device=eng.device)
    p = [x.data_ptr() for x in dw]

    def call(B=1, T=2, gi_p=g.data_ptr(), tag=0, whh_f=p[0]):
        return eng.lib.rvcx_gru_bidir(eng.ctx, gi_p, B, T, whh_f, p[1], p[2], p[3], out.data_ptr(), tag, eng.stream())

    assert call() == 0
    for kw in (dict(B=0), dict(T=0), dict(gi_p=None), dict(tag=2 ** 32), dict(whh_f=p[0] + 4)):
        assert _lib.STATUS[call(**kw)] == "RVCX_E_INVALID", kw
    done(eng)
