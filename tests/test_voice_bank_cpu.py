"""Host side of the voice bank: the planning functions that order a batch's rows by voice and bucket utterances by what
their voices must share (rvcx.offline.order_by_voice / bucket_voices, rvcx.infer.pipeline.voice_key), StreamGroup's
argument checks (rvcx.realtime.slot_voices / zero_rate_without_index), and the new entry points in the header, the
binding table and the library (no compute call: there is no GPU here)."""
import ctypes
import dataclasses

import pytest

from abi_headers import header_prototypes

VOICE_ENTRIES = {"rvcx_voice_new": 2, "rvcx_voice_select": 2, "rvcx_voice_current": 2, "rvcx_voice_info": 3,
                 "rvcx_voice_free": 2, "rvcx_rt_set_voice": 4, "rvcx_rt_get_voices": 2,
                 "rvcx_pipeline_batch_voices": 17}


def test_order_by_voice_keeps_voices_contiguous_and_stable():
    from rvcx.offline import order_by_voice

    voices = {0: "a", 1: "b", 2: "a", 3: "c", 4: "b"}
    assert order_by_voice([0, 1, 2, 3, 4], voices) == [0, 2, 1, 4, 3]
    assert order_by_voice([4, 3, 2, 1, 0], voices) == [4, 1, 3, 2, 0]  # the voices by their first row, rows in order
    assert order_by_voice([2, 0], voices) == [2, 0]  # one voice: the given order
    assert order_by_voice([], voices) == []


def test_bucket_voices_splits_by_key_then_length():
    from rvcx.offline import bucket, bucket_voices

    lengths = [100, 100, 90, 100, 30, 95]
    voices = ["a", "b", "a", "c", "b", "c"]
    keys = {"a": 48, "b": 48, "c": 40}  # c cannot share a pass with a and b
    plan = bucket_voices(lengths, voices, keys, 4, 0.2)
    assert sorted(i for g in plan for i in g) == list(range(6))  # every utterance once
    assert plan == [[0, 2, 1], [4], [3, 5]]
    for g in plan:
        assert len({keys[voices[i]] for i in g}) == 1
        vs = [voices[i] for i in g]
        for v in set(vs):  # the rows of one voice are contiguous
            at = [k for k, x in enumerate(vs) if x == v]
            assert at == list(range(at[0], at[0] + len(at))), (g, vs)
        assert min(lengths[i] for i in g) >= 0.8 * max(lengths[i] for i in g)
    # one voice is bucket itself; a batch limit splits a key's part
    assert bucket_voices(lengths, ["a"] * 6, {"a": 0}, 4, 0.2) == bucket(lengths, 4, 0.2)
    assert [len(g) for g in bucket_voices([10] * 5, list("ababa"), {"a": 0, "b": 0}, 2, 0.0)] == [2, 2, 1]
    with pytest.raises(ValueError):
        bucket_voices(lengths, voices, keys, 0, 0.2)


def test_voice_key_separates_what_one_pass_cannot_share():
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer.pipeline import voice_key

    base = voice_key(SYNTH_48K_V2, False)
    assert base == voice_key(dataclasses.replace(SYNTH_48K_V2, spk_embed_dim=4), False)  # sid range: per row, not shared
    other = [dataclasses.replace(SYNTH_48K_V2, sr=40000, upsample_rates=(10, 10, 2, 2)),
             dataclasses.replace(SYNTH_48K_V2, use_f0=False),
             dataclasses.replace(SYNTH_48K_V2, text_enc_hidden_dim=256),
             dataclasses.replace(SYNTH_48K_V2, vocoder="RefineGAN"),
             dataclasses.replace(SYNTH_48K_V2, inter_channels=96)]
    # the rule names the PRODUCT of the upsample rates: other rates with the same product share a pass
    assert base == voice_key(dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 6, 2, 2, 2)), False)
    keys = {voice_key(c, False) for c in other}
    assert len(keys) == len(other) and base not in keys
    assert voice_key(SYNTH_48K_V2, True) != base  # a voice that retrieves and one that cannot share no index_rate


def test_slot_voices_checks_its_arguments():
    from rvcx.realtime import slot_voices

    assert slot_voices(3, None, 2) == [2, 2, 2]
    assert slot_voices(3, 1, 0) == [1, 1, 1]
    assert slot_voices(3, [0, 2, 0], 0) == [0, 2, 0]
    for bad in ([0, 1], [0, 1, 2, 3], [0, "a", 1], [0, -1, 1], [0, 1.5, 1], [True, 0, 1], "abc"):
        with pytest.raises(ValueError):
            slot_voices(3, bad, 0)


def test_index_rate_is_zeroed_per_voice():
    from rvcx import _lib
    from rvcx.realtime import zero_rate_without_index

    arr = (_lib.RtOpts * 4)()
    for o in arr:
        o.index_rate = 0.5
    zero_rate_without_index(arr, [0, 1, 0, 1], {0: True, 1: False}, [1, 1, 1, 0])
    assert [o.index_rate for o in arr] == [0.5, 0.0, 0.5, 0.5]  # the idle slot's rate is ignored, so left alone
    zero_rate_without_index(arr, [0, 1, 0, 1], {0: False, 1: False})
    assert [o.index_rate for o in arr] == [0.0] * 4


def test_voice_entry_points_are_declared_bound_and_exported():
    from rvcx import _lib

    protos = header_prototypes("rvcx.h")
    lib = _lib.load()
    for name, nargs in VOICE_ENTRIES.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert name in _lib.SIG and len(_lib.SIG[name][1]) == nargs and name not in _lib.TEST_SIG
        assert name in _lib.exported_symbols()
        nulls = [None if issubclass(t, (ctypes._Pointer, ctypes.c_void_p)) else 0 for t in _lib.SIG[name][1]]
        assert _lib.STATUS[getattr(lib, name)(*nulls)] == "RVCX_E_INVALID"  # no context, no group
    # rvcx_voice_desc: the synthesizer descriptor (an even number of ints), two ints and six int64, no padding
    assert ctypes.sizeof(_lib.SynthDesc) % 8 == 0
    assert ctypes.sizeof(_lib.VoiceDesc) == ctypes.sizeof(_lib.SynthDesc) + 2 * 4 + 6 * 8
