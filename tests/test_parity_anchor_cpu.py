"""The anchored bars (tests/parity_anchor.py: K x the oracle's own fp32-vs-fp64 gap) discriminate, no GPU: a deviation
applied to the fp32 oracle, of the kind a device kernel could carry, lands beyond K gap at the shapes
test_gpu_module_fp64.py uses, so that file would fail on it. Also anchor() and check() themselves: the 2^-23 floor,
the absolute mode, the thread-count restore.

Distance to float64 in units of the gap, measured on the CPU oracle with the inputs below (1.0 is the undisturbed
oracle; for the synthesizer the largest of the five outputs the GPU file checks):

    HuBERT n = 400 / 5000 / 10080 / 16000     LayerNorm eps 1e-6   7.3e3 / 2.6e4 / 1.4e4 / 1.4e4
                                              GELU tanh form       411 / 652 / 426 / 378
                                              GroupNorm eps 1e-6   1057 / 347 / 811 / 843
    RMVPE  n = 16000                          BatchNorm eps 1e-6   37 (20 on another clip)
    synth  (B, T) = (1, 1) / (1, 24)          final leaky-ReLU slope 0.1 for the default 0.01   1.2e5 / 2.4e4 (waveform)
                                              every leaky-ReLU slope x (1 + 1e-4)               29 / 21

Not resolved at K = 8, and not asserted. The RMVPE BatchNorm eps on the short clips: 9.2 .. 39 at n = 2720, 5.1 at
4960, 11 at 5280 over two clips each (the gap itself, a maximum over few frames, moves 2.7e-6 .. 4.7e-5 there). The
TextEncoder's LayerNorm eps 1e-6, which the six post-norm layers renormalise away: 40 on z_p at T = 1, but 4.0 at
(1, 24) and 1.2 at (3, 40).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_anchor as pa
from parity_anchor import K, PatchedF, anchor, check, ratios


# ----------------------------------------------------------------- anchor / check themselves
def test_check_floor():
    ref = np.array([1.0, -0.5, 0.25])
    check("floor", ref + 7 * 2.0 ** -23, ref, 0.0, K)  # a zero gap cannot ask for better than fp32 can store
    with pytest.raises(AssertionError):
        check("floor", ref + 9 * 2.0 ** -23, ref, 0.0, K)
    check("gap", ref + 7e-5, ref, 1e-5, K)
    with pytest.raises(AssertionError):
        check("gap", ref + 9e-5, ref, 1e-5, K)
    assert check("gap", ref * 2 + 2e-5, ref * 2, 2e-5, K) == pytest.approx(1e-5)  # err and gap relative to max |ref|


def test_check_absolute_mode():
    ref = np.array([0.01, 0.002])
    dev = ref + 1e-7
    assert check("abs", dev, ref, 0.0, K, absolute=True) == pytest.approx(1e-7)  # <= 8 x 2^-23 of 1.0
    with pytest.raises(AssertionError):
        check("rel", dev, ref, 0.0, K)  # 1e-5 of the peak
    with pytest.raises(AssertionError):
        check("shape", dev[:1], ref, 1.0, K)
    with pytest.raises(AssertionError):
        check("nan", np.array([np.nan, 0.0]), ref, 1.0, K)


def test_check_prints_one_line(capsys):
    check("name", np.ones(3) + 2e-6, np.ones(3), 1e-6, K)
    line = capsys.readouterr().out.strip()
    assert line.startswith("name: err 2.000e-06 bound 8.000e-06 err/gap 2.00"), line


def test_anchor_threads_and_gap():
    seen = []

    def fn(dt):
        seen.append((dt, torch.get_num_threads()))
        v = 0.0 if dt == torch.float64 else 1e-3 * torch.get_num_threads()
        return {"a": torch.full((2, 3), 1.0 + v, dtype=dt), "b": torch.zeros(4, dtype=dt)}

    n0 = torch.get_num_threads()
    torch.set_num_threads(3)
    try:
        anc = anchor(fn)
        assert torch.get_num_threads() == 3
        assert [s[0] for s in seen] == [torch.float64, torch.float32, torch.float32]
        assert [s[1] for s in seen[1:]] == [1, 8]
        ref, gap = anc["a"]
        assert ref.dtype == np.float64 and ref.shape == (2, 3) and gap == pytest.approx(8e-3, rel=1e-4)
        assert anc["b"][1] == 0.0

        def boom(dt):
            if dt == torch.float32:
                raise ValueError("boom")
            return torch.zeros(1, dtype=dt)

        with pytest.raises(ValueError):
            anchor(boom)
        assert torch.get_num_threads() == 3
        assert set(anchor(lambda dt: torch.ones(2, dtype=dt))) == {"out"}
    finally:
        torch.set_num_threads(n0)


def test_cast_weights_floating_only():
    w = {"w": np.ones(3, np.float32), "n": np.array(7, np.int64), "t": torch.ones(2, dtype=torch.float16)}
    c = pa.cast_weights(w, torch.float64)
    assert c["w"].dtype == torch.float64 and c["t"].dtype == torch.float64 and c["n"].dtype == torch.int64
    assert int(c["n"]) == 7 and w["w"].dtype == np.float32


# ----------------------------------------------------------------- the bars discriminate
@pytest.mark.parametrize("n", [400, 5000, 10080, 16000])
def test_hubert_deviations_land_beyond_the_bar(hubert_w, monkeypatch, n):
    from oracle import hubert as ohub
    from rvcx import synthetic

    fn = pa.hubert_fn(hubert_w, synthetic.speech_like(n, seed=40).astype(np.float32)[None])
    anc = anchor(fn)
    assert ratios(fn, anc)["out"] <= 2.0  # any fp32 summation order
    for name, over in (("LayerNorm eps", dict(layer_norm=lambda x, s, g, b, e: F.layer_norm(x, s, g, b, 1e-6))),
                       ("GELU tanh", dict(gelu=lambda x: F.gelu(x, approximate="tanh"))),
                       ("GroupNorm eps", dict(group_norm=lambda x, g_, w, b, e: F.group_norm(x, g_, w, b, 1e-6)))):
        monkeypatch.setattr(ohub, "F", PatchedF(**over))
        r = ratios(fn, anc)["out"]
        monkeypatch.setattr(ohub, "F", F)
        print(f"\nHuBERT n={n} {name}: {r:.1f} x gap")
        assert r > K, (name, r)


@pytest.mark.parametrize("n", [16000])
def test_rmvpe_batchnorm_eps_lands_beyond_the_bar(rmvpe_w, monkeypatch, n):
    from oracle import rmvpe as orm
    from rvcx import synthetic

    fn = pa.rmvpe_fn(rmvpe_w, synthetic.speech_like(n, seed=50).astype(np.float32)[None])
    anc = anchor(fn)
    assert ratios(fn, anc, absolute=True)["out"] <= 2.0

    def bn(w, p, x):
        t = orm._t
        return F.batch_norm(x, t(w, p + ".running_mean"), t(w, p + ".running_var"), t(w, p + ".weight"),
                            t(w, p + ".bias"), False, 0.0, 1e-6)

    monkeypatch.setattr(orm, "_bn", bn)
    r = ratios(fn, anc, absolute=True)["out"]
    print(f"\nRMVPE n={n} BatchNorm eps 1e-6: {r:.1f} x gap")
    assert r > K, r


@pytest.mark.parametrize("lengths", [(1,), (24,)])
def test_synth_leaky_slopes_land_beyond_the_bar(synth_w, monkeypatch, lengths):
    from oracle import synth as osynth

    fn = pa.synth_fn(synth_w, **pa.synth_case(lengths, seed=60))
    anc = anchor(fn)
    assert max(ratios(fn, anc).values()) <= 2.0
    # the generator's last activation is F.leaky_relu(x): torch's default slope 0.01, not the 0.1 of every other one
    monkeypatch.setattr(osynth, "F", PatchedF(leaky_relu=lambda x, s=None: F.leaky_relu(x, 0.1 if s is None else s)))
    r = ratios(fn, anc)
    print(f"\nsynth {lengths} final slope 0.1: {r['o']:.3g} x gap")
    assert r["o"] > K and max(r[k] for k in ("z_p", "z", "m_p", "logs_p")) <= 2.0, r
    monkeypatch.setattr(osynth, "F", PatchedF(leaky_relu=lambda x, s=0.01: F.leaky_relu(x, s * (1 + 1e-4))))
    r = ratios(fn, anc)
    print(f"\nsynth {lengths} slopes x (1 + 1e-4): " + " ".join(f"{k} {v:.1f}" for k, v in r.items()))
    assert max(r.values()) > K, r  # one output over the bar fails the device test, which checks all five
