"""The voice bank (rvcx_voice_new / select / current / info / free): several voice models resident in one context.

* The bank is transparent: an engine that holds voice X (id 0) and voice A (id 1), each with its own index, and has
  selected A gives the bits of an engine that loaded A the old way -- synth_infer, pipeline_ex with retrieval, a ragged
  pipeline_batch_v and a 3-slot stream group -- and again after selecting X and then A. Bar: bit equality (the two
  engines run the same calls in the same order on the same shapes).
* Refusals leave everything usable: unknown ids, voice 0 and the current voice at free, unfinalized and incompatible
  voices in a stream group and in the C batch call, rows of one voice that are not contiguous, a freed voice in an
  active slot, index_rate > 0 on a voice without an index. After every refused call the current voice is the one it was
  and the device status is clean.
* Free gives the memory back: the device's free memory rises by at least the weight_bytes + split_bytes that voice_info
  reported while the voice was resident and had been used once."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from ragged_rows import PIPE_NS, PIPE_SIDS, SHORT_PAD, clip, noise_for
from voice_bank_common import (BLOCK, RVCX_E_INVALID, RVCX_E_SHAPE, RVCX_E_STATE, SEED_A, SEED_B, SEED_X,
                               assert_separated, bank_engine, blocks, group, hop, index_for, noise, weights)

pytestmark = pytest.mark.gpu


def _synth_inputs(T=32, seed=5):
    from rvcx import synthetic

    rng = np.random.Generator(np.random.PCG64(seed))
    phone = rng.standard_normal((1, T, 768)).astype(np.float32)
    pitch = rng.integers(1, 256, size=(1, T)).astype(np.int64)
    eps_z = rng.standard_normal((1, 192, T)).astype(np.float32)
    eps_src = rng.standard_normal((1, T * 480)).astype(np.float32)
    return (phone, [T], pitch, synthetic.f0_walk(1, T, seed=seed + 1), [0]), dict(eps_z=eps_z, eps_src=eps_src)


def _surface(eng):
    """Every entry point the issue names on the engine's current voice -> a dict of numpy results."""
    eng.set_pipeline_highpass()
    res = {}
    args, nz = _synth_inputs()
    res["synth_infer"] = eng.host(eng.synth_infer(*args, **nz))
    a = clip(12000, 41)
    o = eng.pipeline_opts(index_rate=0.5, pitch=2.0, **SHORT_PAD)
    T = eng.pipeline_frames(len(a), o)
    rng = np.random.default_rng(43)
    ez, es = rng.standard_normal(192 * T).astype(np.float32), rng.standard_normal(T * eng.upp).astype(np.float32)
    y, f0 = eng.pipeline_ex(a, o, eps_z=ez, eps_src=es, want_f0=True)
    res["pipeline_ex"], res["pipeline_ex f0"] = eng.host(y), eng.host(f0)
    rows = [clip(n, 50 + b) for b, n in enumerate(PIPE_NS[:3])]
    _, bz, bs = noise_for(eng, rows, o, 47)
    ys = eng.pipeline_batch_v(rows, o, sids=PIPE_SIDS[:3], eps_z=bz, eps_src=bs)
    for b, yb in enumerate(ys):
        res[f"pipeline_batch_v row {b}"] = eng.host(yb)
    grp = group(eng, 3)
    audio = np.stack([blocks(2, 60 + b) for b in range(3)])
    rng = np.random.default_rng(53)
    for h in range(2):
        out, vol, offs, model = hop(eng, grp, audio[:, h], grp.opts(index_rate=0.5, f0_up_key=3), *noise(rng, 3))
        res[f"stream hop {h} out"], res[f"stream hop {h} vol"], res[f"stream hop {h} offs"] = out, vol, offs
    grp.close()
    eng.check_device_status()
    return res


def test_bank_is_transparent(hubert_w, rmvpe_w):
    e1, _ = bank_engine(hubert_w, rmvpe_w, [SEED_A])
    e2, ids = bank_engine(hubert_w, rmvpe_w, [SEED_X, SEED_A])
    try:
        want = _surface(e1)
        assert e2.voice == 0 and e2.voice_ids == [0, 1]
        on_x = _surface(e2)  # voice X: another voice altogether
        assert_separated("synth_infer A / X", want["synth_infer"][0], on_x["synth_infer"][0])
        for round_ in range(2):  # select A; then X and A again
            e2.select_voice(ids[SEED_A])
            assert e2.voice == ids[SEED_A] and e2.index_info()["ntotal"] == index_for(hubert_w, SEED_A)[0].ntotal
            got = _surface(e2)
            assert sorted(got) == sorted(want)
            for k in want:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"round {round_}: {k}")
                assert np.isfinite(want[k]).all(), k
                assert np.any(want[k]) or k.endswith("offs") or k.startswith("stream hop 0"), k  # (SOLA offsets may be 0)
            e2.select_voice(ids[SEED_X])
            again = _surface(e2) if round_ == 0 else None
            if again:
                for k in on_x:
                    np.testing.assert_array_equal(again[k], on_x[k], err_msg=f"voice X after A: {k}")
        info = e2.voice_info(ids[SEED_A])
        assert info["ready"] and info["sr"] == 48000 and info["upp"] == 480 and info["index"]["nlist"] == 6
        assert info["weight_bytes"] > 10 << 20 and info["split_bytes"] > 0
    finally:
        e1.close()
        e2.close()


def _incompatible():
    """Voices a 48 kHz v2 HiFi-GAN group or batch must refuse: another rate and upsampling, no pitch guidance, the v1
    embedding width (tests/synth_configs.py)."""
    from synth_configs import CONFIGS

    from rvcx.config import SYNTH_48K_V2

    return {"v2_40k": CONFIGS["v2_40k"], "no-f0": dataclasses.replace(SYNTH_48K_V2, use_f0=False),
            "v1_48k": CONFIGS["v1_48k"]}


def test_refusals_leave_everything_usable(hubert_w, rmvpe_w):
    from rvcx import _lib

    eng, ids = bank_engine(hubert_w, rmvpe_w, [SEED_A, SEED_B], indexed=False)
    lib, A, B = eng.lib, 0, 1

    def current():
        v = ctypes.c_int(-7)
        assert lib.rvcx_voice_current(eng.ctx, ctypes.byref(v)) == 0
        return v.value

    def refused(rc, code, what):
        assert rc == code, (what, _lib.STATUS.get(rc, rc), lib.rvcx_last_error(eng.ctx))
        assert current() == A and eng.voice == A, what
        eng.check_device_status()

    try:
        eng.set_pipeline_highpass()
        grp = group(eng, 2, voices=[A, B])
        assert grp.voices == [A, B]
        rng = np.random.default_rng(3)
        x = np.stack([blocks(1, 110)[0], blocks(1, 111)[0]])
        ez, es = noise(rng, 2)
        ok = grp.opts(index_rate=0.0)
        first = hop(eng, grp, x, ok, ez, es)
        assert np.isfinite(first[0]).all() and np.any(first[0][0]) and np.any(first[0][1])
        desc = _lib.VoiceDesc()
        # unknown ids
        for what, rc in (("select", lib.rvcx_voice_select(eng.ctx, 99)),
                         ("info", lib.rvcx_voice_info(eng.ctx, 99, ctypes.byref(desc))),
                         ("free", lib.rvcx_voice_free(eng.ctx, 99)),
                         ("rt_set_voice", lib.rvcx_rt_set_voice(eng.ctx, grp.handle, 0, 99)),
                         ("rt_set_voice slot", lib.rvcx_rt_set_voice(eng.ctx, grp.handle, 2, B))):
            refused(rc, RVCX_E_INVALID, what)
        # voice 0 and the current voice stay
        refused(lib.rvcx_voice_free(eng.ctx, 0), RVCX_E_STATE, "free voice 0")
        eng.select_voice(B)
        assert lib.rvcx_voice_free(eng.ctx, B) == RVCX_E_STATE and current() == B
        eng.select_voice(A)
        # an unfinalized voice
        v = ctypes.c_int(0)
        assert lib.rvcx_voice_new(eng.ctx, ctypes.byref(v)) == 0 and v.value == 2 and current() == A
        empty = v.value
        refused(lib.rvcx_rt_set_voice(eng.ctx, grp.handle, 1, empty), RVCX_E_STATE, "unfinalized voice in a slot")
        # the C batch call: one utterance per row, SHORT_PAD
        rows = [clip(n, 70 + b) for b, n in enumerate(PIPE_NS)]
        opts = eng.pipeline_opts(**SHORT_PAD)

        def batch_rc(voices):
            try:
                eng.pipeline_batch_v(rows, opts, sids=0, voices=voices)
            except _lib.RvcxError as e:
                return e.code
            return 0

        refused(batch_rc([A, B, A, B]), RVCX_E_INVALID, "rows of one voice not contiguous")
        refused(batch_rc([A, A, 99, 99]), RVCX_E_INVALID, "unknown voice in a batch")
        refused(batch_rc([A, A, empty, empty]), RVCX_E_STATE, "unfinalized voice in a batch")
        # incompatible voices
        for name, cfg in _incompatible().items():
            vid = eng.add_voice(weights(7, cfg), cfg)
            refused(lib.rvcx_rt_set_voice(eng.ctx, grp.handle, 1, vid), RVCX_E_SHAPE, f"{name} in a slot")
            refused(batch_rc([A, A, vid, vid]), RVCX_E_SHAPE, f"{name} in a batch")
            eng.free_voice(vid)
            refused(lib.rvcx_voice_select(eng.ctx, vid), RVCX_E_INVALID, f"{name}: a freed id stays unknown")
        assert grp.voices == [A, B]
        # index_rate > 0 on a slot whose voice has no index: the library refuses what process() would have zeroed
        arr = (_lib.RtOpts * 2)(ok, ok)
        arr[1].index_rate = 0.5
        xd, ezd, esd = (eng._dev(t, torch.float32) for t in (x, ez, es))

        def raw_hop(a):
            return lib.rvcx_rt_process_v(eng.ctx, grp.handle, xd.data_ptr(), grp.sids, a, None, ezd.data_ptr(),
                                         esd.data_ptr(), ctypes.c_uint64(0), grp.out.data_ptr(), grp.vol.data_ptr(),
                                         grp.offs.data_ptr(), eng.stream())

        refused(raw_hop(arr), RVCX_E_STATE, "index_rate > 0 without an index")
        # a freed voice in an active slot
        C = eng.add_voice(weights(SEED_X))
        grp.set_voice(1, C)
        eng.free_voice(C)
        refused(raw_hop((_lib.RtOpts * 2)(ok, ok)), RVCX_E_STATE, "freed voice in an active slot")
        grp.set_voice(1, B)
        # none of the refused calls touched the state: a fresh group fed the one accepted hop continues alike
        ref = group(eng, 2, voices=[A, B])
        hop(eng, ref, x, ok, ez, es)
        x2 = np.stack([blocks(2, 110)[1], blocks(2, 111)[1]])
        # with an index on voice A alone, process() zeroes the rate of the slot on B (the reference's rule, per voice)
        eng.index_load(index_for(hubert_w, SEED_A)[1])
        asks = grp.opts(index_rate=0.5)
        assert asks.index_rate == 0.5
        refused(raw_hop((_lib.RtOpts * 2)(ok, asks)), RVCX_E_STATE, "index_rate > 0 on the voice without an index")
        got, want_ = hop(eng, grp, x2, [ok, asks], ez, es), hop(eng, ref, x2, ok, ez, es)
        for g, w in zip(got[:3], want_[:3]):
            np.testing.assert_array_equal(g, w)
        assert np.isfinite(got[0]).all() and np.any(got[0][0]) and np.any(got[0][1])
        assert current() == A
        eng.check_device_status()
        grp.close()
        ref.close()
    finally:
        eng.close()


def test_free_gives_the_memory_back(hubert_w, rmvpe_w):
    eng, _ = bank_engine(hubert_w, rmvpe_w, [SEED_A], indexed=False)
    try:
        args, nz = _synth_inputs()
        eng.host(eng.synth_infer(*args, **nz))  # the shared workspace exists before the first reading
        vid = eng.add_voice(weights(SEED_B), index=index_for(hubert_w, SEED_B)[1])
        eng.select_voice(vid)
        eng.host(eng.synth_infer(*args, **nz))  # used once: its split images are built
        eng.select_voice(0)
        info = eng.voice_info(vid)
        torch.cuda.synchronize()
        resident = torch.cuda.mem_get_info(eng.device)[0]
        eng.free_voice(vid)
        freed = torch.cuda.mem_get_info(eng.device)[0] - resident
        print(f"\nweight_bytes {info['weight_bytes']} split_bytes {info['split_bytes']} freed {freed}")
        assert info["weight_bytes"] > 0 and info["split_bytes"] > 0
        assert freed >= info["weight_bytes"] + info["split_bytes"], (freed, info)
        with pytest.raises(Exception):
            eng.voice_info(vid)
        assert eng.voice_ids == [0]
        eng.host(eng.synth_infer(*args, **nz))
    finally:
        eng.close()
