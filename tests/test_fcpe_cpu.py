"""FCPE on the CPU side: the torch restatement (tests/fcpe_ref.py) against the reference's own run
(tests/golden/fcpe_l2.npz, written by make_golden_fcpe.py from rvc/lib/predictors/FCPE.py), the conditions that make
the GPU tests (tests/test_gpu_fcpe.py) meaningful, the checkpoint loader and the post_process restatement."""
import numpy as np
import pytest
import torch

import fcpe_ref as fr
import parity_anchor as pa
from conftest import golden

LENGTHS = (15000, 1000, 400)


@pytest.fixture(scope="module")
def case():
    """Fixture, sizes, fused weights and, per input length, the anchored (float64 output, fp32 gap) of the mel and
    the salience."""
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, fcpe_sizes

    g = golden("fcpe_l2.npz")
    cfg = synthetic.fcpe_config(int(g["n_layers"]), int(g["n_chans"]))
    z = fcpe_sizes(cfg)
    w = check_fcpe_state(synthetic.fcpe_state(int(g["seed"]), int(g["n_layers"]), int(g["n_chans"])), cfg)
    anchors = {}
    for n in LENGTHS:
        a = torch.from_numpy(synthetic.speech_like(n, seed=int(g["audio_seed"])).astype(np.float32))

        def fn(dt, a=a):
            m = fr.mel(z, a.to(dt))
            return {"mel": m, "sal": fr.salience(pa.weights(w, dt), z, m)}

        anchors[n] = pa.anchor(fn)
    return g, cfg, z, w, anchors


@pytest.mark.parametrize("n", LENGTHS)
def test_restatement_matches_the_reference(case, n):
    """fcpe_ref in fp32 vs the reference's fp32 run: two fp32 evaluations of the same operations, each one gap from
    float64, so they differ by at most 2 gaps (mel and salience); the frame count is n // 160 + 1."""
    g, cfg, z, w, anchors = case
    from rvcx import synthetic

    a = torch.from_numpy(synthetic.speech_like(n, seed=int(g["audio_seed"])).astype(np.float32))
    m = fr.mel(z, a)
    s = fr.salience(pa.weights(w, torch.float32), z, m)
    assert m.shape == g[f"mel_{n}"].shape == (n // 160 + 1, 128) and fr.n_frames(z, n) == n // 160 + 1
    for name, got in (("mel", m), ("sal", s)):
        ref64, gap = anchors[n][name]
        want = g[f"{name}_{n}"]
        err = float(np.abs(got.numpy() - want).max())
        print(f"\n{name} n={n}: restatement vs reference {err:.3e}, gap {gap:.3e}")
        assert err <= 2 * max(gap, pa.ULP32 * np.abs(ref64).max()), (name, err, gap)
        assert np.abs(want - ref64).max() <= max(gap, pa.ULP32 * np.abs(ref64).max()) * 2


def test_decoders_match_the_reference(case):
    """decode on the reference's own salience gives its f0 (both decoders), voicing exactly."""
    g, cfg, z, w, _ = case
    for n in LENGTHS:
        sal = torch.from_numpy(g[f"sal_{n}"])
        ct = torch.from_numpy(w["cent_table"])
        f0 = fr.decode(sal, ct, float(g[f"thr_{n}"])).numpy()
        np.testing.assert_array_equal(f0 > 0, g[f"f0_{n}"] > 0)
        np.testing.assert_allclose(f0, g[f"f0_{n}"], rtol=2e-6, atol=0)
        # the fixture's argmax track was taken at the model's last threshold
        f0a = fr.decode(sal, ct, float(g[f"thr_{n}"]), "argmax").numpy()
        np.testing.assert_allclose(f0a, g[f"f0_argmax_{n}"], rtol=2e-6, atol=0)
        F = sal.shape[0]
        for p_len in (F - 1, F, 2 * F):
            np.testing.assert_allclose(fr.post_process(g[f"f0_{n}"], 160, 16000, p_len), g[f"interp_{n}_{p_len}"],
                                       rtol=1e-12, atol=0)


def test_conditions_of_the_gpu_tests(case):
    """On the float64 reference at n = 15000 (94 frames): the peak bin moves (>= 20 distinct bins), the median
    threshold splits the frames (voiced share in [0.2, 0.8]), the keys' exponent stays far from exp's overflow
    (max(dash_k - diag_k) < 20), fp32 finds the fp64 peak on >= 99 % of the frames, and at most 2 % of the frames lie
    within K gaps of a decision (top-2 margin or threshold): the frames the device test excludes."""
    g, cfg, z, w, anchors = case
    from rvcx import synthetic

    n = 15000
    sal64, gap = anchors[n]["sal"]
    assert sal64.shape == (94, 360)
    peaks = sal64.argmax(1)
    assert len(np.unique(peaks)) >= 20, len(np.unique(peaks))
    mx = g[f"sal_{n}"].max(1)
    thr = float(np.median(mx))
    assert thr == float(g[f"thr_{n}"])
    voiced = float((sal64.max(1) > thr).mean())
    assert 0.2 <= voiced <= 0.8, voiced
    a = torch.from_numpy(synthetic.speech_like(n, seed=int(g["audio_seed"])).astype(np.float64))
    taps = []
    fr.salience_from_audio(pa.weights(w, torch.float64), z, a, taps)
    assert len(taps) == z["n_layers"]
    top = max(float(fr.dash_minus_diag_k(k, P).max()) for _, k, _, P in taps)
    print(f"\nmax(dash_k - diag_k) = {top:.2f}, gap {gap:.3e}, threshold {thr:.4f}, voiced {voiced:.2f}, "
          f"{len(np.unique(peaks))} peak bins")
    assert top < 20.0, top
    s32 = fr.salience_from_audio(pa.weights(w, torch.float32), z, a.float()).numpy()
    assert (s32.argmax(1) == peaks).mean() >= 0.99
    srt = np.sort(sal64, axis=1)
    near = (srt[:, -1] - srt[:, -2] < pa.K * gap) | (np.abs(sal64.max(1) - thr) < pa.K * gap)
    assert near.mean() <= 0.02, near.mean()


def test_load_fcpe_weights_round_trip_and_refusals(case, tmp_path):
    """A checkpoint in FCPE.py's own format round-trips (weight-norm fused, under both spellings); a dict without
    "config" (torchfcpe's bundled format), use_full, a missing tensor and a wrong shape are refused."""
    g, cfg, z, w, _ = case
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, load_fcpe_weights

    raw = synthetic.fcpe_state(int(g["seed"]), int(g["n_layers"]), int(g["n_chans"]))
    sd = {k: torch.from_numpy(v) for k, v in raw.items()}
    p = str(tmp_path / "fcpe.pt")
    torch.save({"config": cfg, "model": sd}, p)
    st, cfg2 = load_fcpe_weights(p)
    assert cfg2 == cfg and set(st) == set(w)
    for k in w:
        np.testing.assert_array_equal(st[k], w[k])
    v, gg = raw["dense_out.parametrizations.weight.original1"], raw["dense_out.parametrizations.weight.original0"]
    want = gg.astype(np.float64) * v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    np.testing.assert_allclose(st["dense_out.weight"], want, rtol=1e-6)
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1",
                                                                              "weight_v"): x for k, x in raw.items()}
    np.testing.assert_array_equal(check_fcpe_state(old, cfg)["dense_out.weight"], st["dense_out.weight"])
    torch.save({"model": sd}, p)
    with pytest.raises(ValueError, match="not an FCPE checkpoint"):
        load_fcpe_weights(p)
    bad = synthetic.fcpe_config(int(g["n_layers"]), int(g["n_chans"]))
    bad["model"]["use_full"] = True
    torch.save({"config": bad, "model": sd}, p)
    with pytest.raises(ValueError, match="use_full"):
        load_fcpe_weights(p)
    with pytest.raises(ValueError, match="missing"):
        check_fcpe_state({k: x for k, x in raw.items() if k != "norm.bias"}, cfg)
    with pytest.raises(ValueError, match="shape"):
        check_fcpe_state(raw, synthetic.fcpe_config(int(g["n_layers"]), 256))
    with pytest.raises(ValueError, match="missing"):
        check_fcpe_state(raw, synthetic.fcpe_config(3, int(g["n_chans"])))
    wide = synthetic.fcpe_config(2, 512)
    wide["model"]["input_channel"] = 80
    with pytest.raises(ValueError, match="input_channel"):
        check_fcpe_state(raw, wide)


def test_post_process_edge_cases():
    """All-unvoiced -> zeros; one voiced frame -> that value everywhere; pad_to != F expands by nearest index first;
    voiced frames keep their values and the ends hold the first / last voiced value."""
    z = np.zeros(9, np.float32)
    np.testing.assert_array_equal(fr.post_process(z, 160, 16000), np.zeros(9))
    np.testing.assert_array_equal(fr.post_process(z, 160, 16000, 5), np.zeros(5))
    one = z.copy()
    one[4] = 220.0
    np.testing.assert_array_equal(fr.post_process(one, 160, 16000, 12), np.full(12, 220.0))
    f0 = np.array([0, 0, 100, 0, 0, 0, 200, 150, 0], np.float32)
    out = fr.post_process(f0, 160, 16000)
    np.testing.assert_allclose(out, [100, 100, 100, 125, 150, 175, 200, 150, 150], rtol=1e-12)
    out = fr.post_process(f0, 160, 16000, 18)  # every frame twice, then interpolated over the doubled grid
    assert out.shape == (18,) and out[4] == out[5] == 100 and out[0] == 100 and out[-1] == 150
    np.testing.assert_allclose(out[6:12], 100 + 100 * np.arange(1, 7) / 7.0, rtol=1e-12)
    out = fr.post_process(f0, 160, 16000, 8)  # F - 1 frames: source index floor(i * 9 / 8)
    src = np.minimum(np.floor(np.arange(8) * np.float32(9 / 8)).astype(int), 8)
    np.testing.assert_array_equal(out[f0[src] > 0], f0[src][f0[src] > 0])
