"""A voice per stream slot (rvcx_rt_set_voice, StreamGroup(voices=) / set_voice): one hop serves several voices, the
front end once over all rows, retrieval and the synthesizer once per voice on its row range.

Voices A, B, C are synthetic.synth_state(2 / 3 / 21) at SYNTH_48K_V2, each with a small IVF index of its own. Geometry
of the existing stream tests: read_chunk_size 96 -> 87 frames, 12288-sample blocks; noise is injected and indexed by
slot.

* mixed group against the oracle: B = 4, slot voices [A, B, A, B] (interleaved, so the row map is not the identity),
  one option set per slot, 3 hops, against one OracleVoiceChanger per stream with that stream's weights and index at the
  bars of test_gpu_stream.py (vol rel <= 1e-5, per-hop correlation > 0.99, SOLA offsets equal on >= 75 % of the
  non-silent hops); and each slot's model row against the same slot of a uniform 4-slot group on that slot's voice at
  ragged_rows.compare_row's bars (correlation > 0.999, difference < 5e-3 of the peak): the front end is the same, only
  the synthesizer's batch size differs.
* isolation: A's slots of [A, B, A, B] equal A's slots of [A, C, A, C] bit for bit in out, vol and offs over 3 hops (same
  group order, positions and group sizes), and again with slot 2 idle.
* switching: a slot moved from A to B without a reset meets the model-row bars against B from the next hop on; after
  reset(stream=i) plus set_voice it equals a fresh group with the same voices, bit for bit."""
import numpy as np
import pytest

from ragged_rows import compare_row
from voice_bank_common import (SEED_A, SEED_B, SEED_C, WINDOW, Bars, assert_separated, bank_engine, blocks, compact_rows,
                               group, hop, index_for, noise, oracle_changer, weights)

pytestmark = pytest.mark.gpu

HOPS = 3
# one option set per slot (StreamGroup.opts / OracleVoiceChanger.on_request keywords): the three of
# test_gpu_stream_slots.py's MIXED and a fourth that retrieves from voice B's index
OPTS = (
    dict(f0_up_key=7, protect=0.33, index_rate=0.6),
    dict(f0_autotune=True, f0_autotune_strength=0.7, index_rate=0.0, volume_envelope=0.4),
    dict(f0_up_key=-3, proposed_pitch=True, proposed_pitch_threshold=200.0, index_rate=1.0),
    dict(f0_up_key=2, protect=0.4, index_rate=0.7),
)
SEEDS = (SEED_A, SEED_B, SEED_A, SEED_B)  # the interleaved group's slot voices


@pytest.fixture(scope="module")
def bank(hubert_w, rmvpe_w):
    eng, ids = bank_engine(hubert_w, rmvpe_w, [SEED_A, SEED_B, SEED_C])
    yield eng, ids
    eng.close()


@pytest.fixture(scope="module")
def inputs():
    audio = np.stack([blocks(HOPS, 60 + b) for b in range(4)])  # [4, HOPS, BLOCK]
    rng = np.random.default_rng(7)
    return audio, [noise(rng, 4) for _ in range(HOPS)]


def _run(eng, voices, inputs, active=None):
    """HOPS hops of a 4-slot group on `voices` with OPTS -> the per-hop (out, vol, offs, model rows)."""
    audio, nz = inputs
    grp = group(eng, 4, voices=voices)
    assert grp.voices == list(voices)
    opts = [grp.opts(**kw) for kw in OPTS]
    assert [o.index_rate for o in opts] == [0.6, 0.0, 1.0, 0.7]
    res = [hop(eng, grp, audio[:, h], opts, *nz[h], active=active) for h in range(HOPS)]
    grp.close()
    assert eng.voice == 0  # a hop leaves the current voice as it found it
    return res


@pytest.fixture(scope="module")
def mixed_run(bank, inputs):
    eng, ids = bank
    return _run(eng, [ids[s] for s in SEEDS], inputs)


@pytest.fixture(scope="module")
def uniform_runs(bank, inputs):
    """The same inputs, options and noise on a uniform 4-slot group per voice."""
    eng, ids = bank
    return {s: _run(eng, [ids[s]] * 4, inputs) for s in (SEED_A, SEED_B)}


def test_mixed_group_model_rows_match_uniform_groups(bank, mixed_run, uniform_runs):
    _, ids = bank
    row = compact_rows([ids[s] for s in SEEDS])
    assert row == {0: 0, 2: 1, 1: 2, 3: 3}  # the voices by their lowest slot, the slots of a voice in order
    h = HOPS - 1
    for b in range(4):  # the two voices tell each other apart on every row before the bars below are trusted
        assert_separated(f"slot {b}", uniform_runs[SEED_A][h][3][b], uniform_runs[SEED_B][h][3][b])
    failed = []
    for h in range(HOPS):
        for b, s in enumerate(SEEDS):
            failed += compare_row(f"hop {h} slot {b}", mixed_run[h][3][row[b]], uniform_runs[s][h][3][b])
            # vol is the front end's alone: the same bits whatever the voices
            assert mixed_run[h][1][b] == uniform_runs[s][h][1][b]
    assert not failed, "; ".join(failed)


def test_mixed_group_matches_oracle(inputs, mixed_run, uniform_runs, hubert_w, rmvpe_w):
    audio, nz = inputs
    assert_separated("slot 0", uniform_runs[SEED_A][HOPS - 1][3][0], uniform_runs[SEED_B][HOPS - 1][3][0])
    bars = Bars()
    for b, (s, kw) in enumerate(zip(SEEDS, OPTS)):
        index = index_for(hubert_w, s)[0] if kw["index_rate"] > 0 else None
        orc = oracle_changer(weights(s), hubert_w, rmvpe_w, b, index)
        for h in range(HOPS):
            out, vol, offs, _ = mixed_run[h]
            bars.hop(orc, audio[b, h], nz[h][0][b], nz[h][1][b], kw, out[b], vol[b], offs[b], (b, h))
    bars.finish()


@pytest.mark.parametrize("active", [None, [True, True, False, True]], ids=["all", "slot2-idle"])
def test_a_voice_is_isolated_from_the_others(bank, inputs, mixed_run, active):
    """A's slots do not see which voice the other slots run: [A, B, A, B] against [A, C, A, C]."""
    eng, ids = bank
    A, B, C = ids[SEED_A], ids[SEED_B], ids[SEED_C]
    with_b = mixed_run if active is None else _run(eng, [A, B, A, B], inputs, active)
    with_c = _run(eng, [A, C, A, C], inputs, active)
    a_slots = [b for b in (0, 2) if active is None or active[b]]
    row_b, row_c = compact_rows([A, B, A, B], active), compact_rows([A, C, A, C], active)
    assert row_b == row_c
    for h in range(HOPS):
        for b in a_slots:
            for k, name in enumerate(("out", "vol", "offs")):
                np.testing.assert_array_equal(with_b[h][k][b], with_c[h][k][b], err_msg=f"hop {h} slot {b} {name}")
            np.testing.assert_array_equal(with_b[h][3][row_b[b]], with_c[h][3][row_c[b]])
            assert np.any(with_b[h][0][b]) or h == 0
        if active is not None:  # the idle slot's contract
            assert not np.any(with_b[h][0][2]) and with_b[h][1][2] == 0 and with_b[h][2][2] == 0
    # B and C really differ where they ran
    assert_separated("slot 1 under B / C", with_b[HOPS - 1][3][row_b[1]], with_c[HOPS - 1][3][row_c[1]])


def test_switching_voice_and_reset(bank):
    eng, ids = bank
    A, B, C = ids[SEED_A], ids[SEED_B], ids[SEED_C]
    n = 6
    audio = np.stack([blocks(n, 80 + b) for b in range(2)])
    rng = np.random.default_rng(19)
    nz = [noise(rng, 2) for _ in range(n)]
    kw = dict(f0_up_key=3, index_rate=0.4)
    P, U = group(eng, 2, voices=A), group(eng, 2, voices=B)
    assert P.voices == [A, A] and U.voices == [B, B]
    rp, ru = [], []
    for h in range(4):
        if h == 2:
            P.set_voice(1, B)  # no reset: the slot keeps its buffers and its SOLA tail
            assert P.voices == [A, B]
        rp.append(hop(eng, P, audio[:, h], P.opts(**kw), *nz[h]))
        ru.append(hop(eng, U, audio[:, h], U.opts(**kw), *nz[h]))
    # without a volume envelope or a noise gate the generator writes only the samples SOLA reads (the output window):
    # the rest of a model row is unspecified, so the rows are compared over the window
    W = WINDOW
    assert_separated("slot 1 on A / on B", rp[1][3][1][:W], ru[1][3][1][:W])
    failed = []
    for h in (2, 3):  # from the next hop on the slot is B's: the front-end state does not depend on the voice
        failed += compare_row(f"switched slot, hop {h}", rp[h][3][1][:W], ru[h][3][1][:W])
    assert not failed, "; ".join(failed)
    # a newcomer: reset plus set_voice equals a fresh group with the same voices, bit for bit
    P.reset(stream=1)
    P.set_voice(1, C)
    F = group(eng, 2, voices=[A, C])
    for h in (4, 5):
        got = hop(eng, P, audio[:, h], P.opts(**kw), *nz[h])
        want = hop(eng, F, audio[:, h], F.opts(**kw), *nz[h])
        for k, name in enumerate(("out", "vol", "offs")):
            np.testing.assert_array_equal(got[k][1], want[k][1], err_msg=f"hop {h} {name}")
        np.testing.assert_array_equal(got[3][1][:W], want[3][1][:W], err_msg=f"hop {h} model row")
        assert np.isfinite(got[0]).all() and (np.any(got[0][1]) or h == 4)
    eng.check_device_status()
    for g in (P, U, F):
        g.close()
