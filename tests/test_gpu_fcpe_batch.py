"""The batched FCPE forward (rvcx_fcpe_b, Engine.fcpe_batch): B streams in one set of launches per layer, as a realtime
hop with f0_method "fcpe" runs it. What the network pads or reduces over time must stay each stream's own: the
Performer attention's ksum / ctx / row maximum / denominator, the GroupNorm statistics, the depthwise conv's and the
k = 3 convs' zero padding, the reflect- or zero-padded STFT framing and the repeated last mel frame.

Bounds are those of tests/test_gpu_fcpe.py (tests/parity_anchor.py): the device stays within K = 8 times the distance
of an honest fp32 evaluation from float64 on the same stream alone. A statistic or a padded tap shared between
streams misses that by orders of magnitude; the independence test then demands bit equality of one stream's result
whatever its neighbours hold."""
import numpy as np
import pytest
import torch

import fcpe_ref as fr
import parity_anchor as pa
from conftest import golden
from fcpe_ref import ATTN_D as D, ATTN_H as H, ATTN_M as M, attention_operands as _attention_operands

pytestmark = pytest.mark.gpu

B = 3
SCALES = (1.0, 0.3, 2.0)  # per stream, so the GroupNorm statistics differ visibly
# 400: 3 frames, the zero-padding branch, shorter than the depthwise kernel; 1000: 7 frames, reflect padding;
# 13920: the realtime convert buffer, 87 STFT frames and 88 output frames; 48000: 301 frames, three attention slabs
LENGTHS = (400, 1000, 13920, 48000)


def _streams(n, seeds=(7, 8, 9), scales=SCALES):
    from rvcx import synthetic

    return np.stack([(synthetic.speech_like(n, seed=s) * k).astype(np.float32) for s, k in zip(seeds, scales)])


@pytest.fixture(scope="module")
def model(engine):
    """The seeded 2-layer, 512-channel model of fcpe_l2.npz on the session engine, and a cache of per-length results:
    the streams, each stream's anchored float64 salience with its own fp32 gap, and the device's batched salience."""
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, fcpe_sizes

    g = golden("fcpe_l2.npz")
    cfg = synthetic.fcpe_config(int(g["n_layers"]), int(g["n_chans"]))
    raw = synthetic.fcpe_state(int(g["seed"]), int(g["n_layers"]), int(g["n_chans"]))
    engine.load_fcpe(raw, cfg)
    return dict(z=fcpe_sizes(cfg), w=check_fcpe_state(raw, cfg), cache={})


def _case(engine, model, n):
    if n not in model["cache"]:
        x = _streams(n)
        refs = []
        for b in range(B):
            a = torch.from_numpy(x[b])
            refs.append(pa.anchor(lambda dt, a=a: fr.salience_from_audio(pa.weights(model["w"], dt), model["z"],
                                                                         a.to(dt)))["out"])
        f0, sal = engine.fcpe_batch(x, 0.5, want_salience=True)
        model["cache"][n] = (x, refs, sal.cpu().numpy())
    return model["cache"][n]


# ---------------------------------------------------------------- Performer attention, kernel level
@pytest.mark.parametrize("T", [7, 94, 301])
def test_batched_attention_is_fp32_accurate_per_stream(engine, T):
    """B = 3 streams with different operands in one call, T = 7 (below one 16-row time tile), 94 (ragged single slab),
    301 (three 128-row slabs, the last ragged): each stream within K gaps of float64 on its own operands. ctx, ksum,
    the row maximum or the denominator taken over more than one stream would be off by order 1."""
    ops = [_attention_operands(T, 1.0, 5000 * T + b) for b in range(B)]
    P = ops[0][3]
    q, k, v = (np.stack([o[i] for o in ops]) for i in range(3))
    assert q.shape == (B, H, T, D) and P.shape == (M, D)
    out = engine.performer_attention_batch(q, k, v, P)
    t = torch.from_numpy
    points = []
    for b in range(B):
        ref64, gap = pa.anchor(lambda dt, b=b: fr.performer_attention(t(q[b]).to(dt), t(k[b]).to(dt), t(v[b]).to(dt),
                                                                      t(P).to(dt)))["out"]
        points.append((f"batched performer T={T} stream {b}", out[b], ref64, gap, pa.K))
    pa.check_each(points)
    if T == 301:  # the slabs of every (stream, head) are combined in slab order, without atomics
        assert torch.equal(engine.performer_attention_batch(q, k, v, P), out)


# ---------------------------------------------------------------- salience per stream
@pytest.mark.parametrize("n", LENGTHS)
def test_salience_per_stream_vs_fp64(engine, model, n):
    """Each row of the batched salience within K gaps (absolute: the outputs live in [0, 1]) of the float64
    restatement run on that stream alone; the gap is that stream's own anchor."""
    x, refs, sal = _case(engine, model, n)
    F = n // 160 + 1
    assert sal.shape == (B, F, 360)
    pa.check_each([(f"fcpe_batch salience n={n} stream {b} (x{SCALES[b]:g})", sal[b], refs[b][0], refs[b][1], pa.K, True)
                   for b in range(B)])


# ---------------------------------------------------------------- independence
@pytest.mark.parametrize("n", LENGTHS)
def test_stream_is_independent_of_its_neighbours(engine, model, n):
    """(a, b, c) against (a', b, c') with the neighbours replaced by other seeds and scales: stream b's salience and f0
    are bit-identical, with b in the middle, first and last."""
    xa = _streams(n)
    xb = _streams(n, seeds=(21, 8, 23), scales=(2.5, 0.3, 0.1))
    for pos in (1, 0, 2):
        order = [1, 0, 2] if pos == 0 else [0, 2, 1] if pos == 2 else [0, 1, 2]
        assert order[pos] == 1
        f1, s1 = engine.fcpe_batch(xa[order], 0.5, want_salience=True)
        f2, s2 = engine.fcpe_batch(xb[order], 0.5, want_salience=True)
        assert torch.equal(s1[pos], s2[pos]) and torch.equal(f1[pos], f2[pos]), (n, pos)
        for other in range(B):
            if other != pos:
                assert not torch.equal(s1[other], s2[other])


# ---------------------------------------------------------------- f0
@pytest.mark.parametrize("n", LENGTHS)
def test_f0_rows_decode_their_own_salience(engine, model, n):
    """f0 [B][F] is the local_argmax decode of the device's own salience rows (voicing exact, rtol 2e-6), holds fp32
    values, and at the median of the frame maxima every stream has a voiced share in [0.2, 0.8]."""
    x, _, sal0 = _case(engine, model, n)
    thr = float(np.float32(np.median(sal0.max(2))))
    f0, sal = engine.fcpe_batch(x, thr, want_salience=True)
    f0, sal = f0.cpu().numpy(), sal.cpu().numpy()
    assert np.array_equal(sal, sal0)
    assert f0.shape == (B, n // 160 + 1)
    cent = torch.from_numpy(model["w"]["cent_table"])
    for b in range(B):
        want = fr.decode(torch.from_numpy(sal[b]), cent, thr).numpy()
        np.testing.assert_array_equal(f0[b] > 0, want > 0)
        np.testing.assert_allclose(f0[b], want, rtol=2e-6, atol=0)
        share = float((f0[b] > 0).mean())
        print(f"\nfcpe_batch n={n} stream {b}: voiced share {share:.2f} at threshold {thr:.4f}")
        assert 0.2 <= share <= 0.8, (n, b, share)
    assert np.array_equal(f0.astype(np.float32).astype(np.float64), f0)  # the raw track holds fp32 values
