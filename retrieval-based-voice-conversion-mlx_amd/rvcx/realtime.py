"""Streaming voice conversion on MI355X (config C5) -- the rvc/realtime surface.

Mirrors rvc/realtime/core.py (``VoiceChanger`` :329-484 with ``process_audio`` / ``on_request``,
``Realtime`` :36-326) and the per-hop semantics of rvc/realtime/pipeline.py (``Realtime_Pipeline``
:99-352). The MLX port of this path (rvc_mlx/realtime) is not functional, so the
PyTorch path's behaviour is the contract.

``StreamGroup`` converts B concurrent streams of one geometry per hop in one device call
(``rvcx_rt_process_v``: resample, circular buffers, RMS gate, RMVPE or FCPE (``f0_method``), HuBERT, retrieval, one batched
Synthesizer.infer, SOLA crossfade -- all HIP kernels). ``VoiceChanger`` is the one-stream, numpy-in /
numpy-out object of the reference. The noise gate of ``Realtime(..., clean_audio=True, clean_strength=...)``
(core.py:86-94, pipeline.py:326-327) is a setting of each stream (``rvcx_rt_set_clean``), carried here by the options. Audio I/O, VAD and pedalboard effects are CPU
libraries and not part of this path: ``vad_enabled=True`` / ``post_process=True`` raise instead of being dropped.

A group's B slots are independent users: every hop takes one ``RtOpts`` for all of them or one per slot (each slot its
own ``on_request`` arguments), a set of slots may sit a hop out (``active``), and ``reset(stream=i)`` clears one slot
for a newcomer without touching the others.
"""
from __future__ import annotations

import ctypes
import time
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .engine import Engine

F0_METHODS = ("rmvpe", "fcpe")  # VoiceChanger's f0_method (rvc/realtime/pipeline.py:140-155)


def _f0_method_id(f0_method) -> int:
    if f0_method not in F0_METHODS:
        raise ValueError(f"f0_method {f0_method!r} is not supported in realtime streams: one of {F0_METHODS}")
    return F0_METHODS.index(f0_method)


GEOMETRY_FIELDS = ("n_streams", "block48", "block16", "convert16", "frames", "skip_head", "return_length",
                   "crossfade48", "sola_search48", "extra48", "resampled_block16", "silence_front")


def _ptr(t):
    return None if t is None else t.data_ptr()


def hop_arguments(n_streams: int, opts, active=None):
    """The per-slot arguments of one hop, checked on the host: ``opts`` one ``RtOpts`` (every slot) or a sequence of
    ``n_streams`` of them, ``active`` None (every slot) or a sequence of ``n_streams`` booleans. Returns (a ctypes
    array of n_streams RtOpts, a ctypes uint8 array or None). ValueError for a wrong length or when the active slots
    disagree on gen_precision (one hop runs one generator precision)."""
    if isinstance(opts, _lib.RtOpts):
        each = [opts] * n_streams
    else:
        each = list(opts)
        if len(each) != n_streams:
            raise ValueError(f"opts has {len(each)} entries for {n_streams} streams")
        if not all(isinstance(o, _lib.RtOpts) for o in each):
            raise ValueError("opts must be RtOpts (StreamGroup.opts) or a sequence of them")
    act = None
    if active is not None:
        flags = [bool(a) for a in active]
        if len(flags) != n_streams:
            raise ValueError(f"active has {len(flags)} entries for {n_streams} streams")
        act = (ctypes.c_uint8 * n_streams)(*[int(a) for a in flags])
    else:
        flags = [True] * n_streams
    precisions = {int(o.gen_precision) for o, a in zip(each, flags) if a}
    if len(precisions) > 1:
        raise ValueError("the active streams of one hop must agree on gen_precision")
    return (_lib.RtOpts * n_streams)(*each), act  # the array holds copies


def check_clean_strength(clean_strength) -> float:
    """clean_strength as TorchGate's prop_decrease: a float in [0, 1], or ValueError (TorchGate asserts it)."""
    v = float(clean_strength)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"clean_strength must lie in [0, 1], got {clean_strength!r}")
    return v


def check_slot(n_streams: int, stream) -> int:
    """A slot index of a group of n_streams, or ValueError."""
    if isinstance(stream, bool) or int(stream) != stream or not 0 <= int(stream) < n_streams:
        raise ValueError(f"stream {stream!r} is not a slot of a {n_streams}-stream group")
    return int(stream)


def slot_voices(n_streams: int, voices, current: int):
    """The voice id of each slot, checked on the host: ``voices`` None (every slot on ``current``), one id (every
    slot on it) or a sequence of ``n_streams`` ids. ValueError for a wrong length or something that is no id."""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
            raise ValueError(f"voice {v!r} is not a voice id (Engine.add_voice returns them)")
        return int(v)

    if voices is None:
        return [int(current)] * n_streams
    if isinstance(voices, (int, np.integer)):
        return [one(voices)] * n_streams
    each = [one(v) for v in voices]
    if len(each) != n_streams:
        raise ValueError(f"voices has {len(each)} entries for {n_streams} streams")
    return each


def zero_rate_without_index(arr, voices, has_index, active=None):
    """rvc/realtime only retrieves when an index is loaded (pipeline.py:264), here per voice: the index_rate of every
    active slot whose voice has no index becomes 0, in place in the ctypes array ``arr``. ``has_index``: voice id ->
    bool."""
    for b, v in enumerate(voices):
        if (active is None or active[b]) and arr[b].index_rate > 0 and not has_index[v]:
            arr[b].index_rate = 0.0
    return arr


class StreamGroup:
    """B streams sharing one buffer geometry, converted together each hop on one Engine.

    voices: the voice of each slot (``Engine.add_voice`` ids): None = the Engine's current voice, one id, or one per
    slot. The group takes its geometry from the first slot's voice; every other voice must agree with it on the
    sampling rate, the upsample product, the embedding width, inter_channels, pitch guidance and the vocoder
    (RvcxError RVCX_E_SHAPE otherwise). A slot keeps its voice whatever ``Engine.select_voice`` does later;
    ``set_voice`` changes it. The hop runs the pitch network and HuBERT once over all slots and the synthesizer once per
    voice in use.

    f0_method "rmvpe" (the default) or "fcpe": the pitch network every hop runs, batched over the B convert buffers.
    "fcpe" uses the checkpoint loaded with ``Engine.load_fcpe`` (16 kHz, hop 160) and needs no RMVPE weights; its raw
    local_argmax track is voiced where the frame maximum exceeds fcpe_threshold (the reference's 0.006).

    clean_audio / clean_strength: the defaults ``opts()`` fills in -- the noise gate of Realtime(..., clean_audio=True,
    clean_strength=0.5) on each stream's model output; ``opts(clean_audio=..., clean_strength=...)`` overrides them per
    stream."""

    def __init__(self, engine: Engine, n_streams: int = 1, read_chunk_size: int = 192,
                 cross_fade_overlap_size: float = 0.1, extra_convert_size: float = 0.5,
                 silent_threshold: float = -90.0, sid=0, f0_method: str = "rmvpe", fcpe_threshold: float = 0.006,
                 clean_audio: bool = False, clean_strength: float = 0.5, voices=None):
        method = _f0_method_id(f0_method)
        n_streams = int(n_streams)
        voices = slot_voices(n_streams, voices, engine.voice)
        self.clean_audio, self.clean_strength = bool(clean_audio), check_clean_strength(clean_strength)
        if f0_method == "fcpe" and getattr(engine, "fcpe_cfg", None) is None:
            raise ValueError('f0_method "fcpe" needs an FCPE checkpoint on the Engine (Engine.load_fcpe)')
        self.engine = engine
        self.f0_method = f0_method
        lib = engine.lib
        d = _lib.RtDesc()
        lib.rvcx_rt_default_desc(ctypes.byref(d))
        d.n_streams, d.read_chunk_size = int(n_streams), int(read_chunk_size)
        d.cross_fade_overlap_size, d.extra_convert_size = float(cross_fade_overlap_size), float(extra_convert_size)
        d.silent_threshold = float(silent_threshold)
        d.f0_method, d.fcpe_threshold = method, float(fcpe_threshold)
        h = ctypes.c_void_p()
        # the group takes its geometry from the first slot's voice (rvcx_rt_create reads the current one)
        back = engine.voice
        if voices[0] != back:
            engine.select_voice(voices[0])
        try:
            engine._check(lib.rvcx_rt_create(engine.ctx, ctypes.byref(d), ctypes.byref(h)), "rt_create")
        finally:
            if voices[0] != back:
                engine.select_voice(back)
        self.handle = h
        try:
            for b, v in enumerate(voices):
                if v != voices[0]:
                    engine._check(lib.rvcx_rt_set_voice(engine.ctx, h, b, v), "rt_set_voice")
        except Exception:
            self.close()
            raise
        g = (ctypes.c_int64 * 12)()
        engine._check(lib.rvcx_rt_geometry(h, g), "rt_geometry")
        self.geometry = dict(zip(GEOMETRY_FIELDS, list(g)))
        self.n_streams = self.geometry["n_streams"]
        self.block_frame = self.geometry["block48"]
        sids = np.broadcast_to(np.asarray(sid, dtype=np.int32), (self.n_streams,))
        self.sids = (ctypes.c_int32 * self.n_streams)(*[int(v) for v in sids])
        t = engine.torch
        self.out = t.empty((self.n_streams, self.block_frame), dtype=t.float32, device=engine.device)
        self.vol = t.empty((self.n_streams,), dtype=t.float32, device=engine.device)
        self._clean = [(0, 0.5)] * self.n_streams  # what the library holds per slot (rvcx_rt_set_clean); created off
        self.offs = t.empty((self.n_streams,), dtype=t.int32, device=engine.device)

    def close(self):
        if getattr(self, "handle", None):
            self.engine.lib.rvcx_rt_destroy(self.engine.ctx, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def voices(self):
        """The voice id of each slot (rvcx_rt_get_voices)."""
        out = (ctypes.c_int32 * self.n_streams)()
        self.engine._check(self.engine.lib.rvcx_rt_get_voices(self.handle, out), "rt_get_voices")
        return [int(v) for v in out]

    def set_voice(self, stream: Optional[int], voice: int):
        """Move one slot (``stream=None``: every slot) to another resident voice. The slot's buffers are kept: a user
        who switches voice keeps the SOLA crossfade, a newcomer also calls ``reset(stream=i)``. RvcxError for a voice
        that does not fit the group (RVCX_E_SHAPE), does not exist (RVCX_E_INVALID) or is not loaded (RVCX_E_STATE);
        the slot then keeps its voice."""
        eng = self.engine
        slot = -1 if stream is None else check_slot(self.n_streams, stream)
        vid = slot_voices(1, voice, 0)[0]
        eng._check(eng.lib.rvcx_rt_set_voice(eng.ctx, self.handle, slot, vid), "rt_set_voice")

    def _has_index(self, voices):
        eng = self.engine
        return {v: (eng.index_info() if v == eng.voice else eng.voice_info(v)["index"]) is not None
                for v in set(voices)}

    def reset(self, stream: Optional[int] = None):
        """Clear the whole group (``stream=None``) or one slot: its audio / convert / pitch buffers and SOLA tail go
        back to zeros, asynchronously on the current stream, and no other slot is touched -- for a user who takes over
        a slot another one left."""
        eng = self.engine
        if stream is None:
            eng._check(eng.lib.rvcx_rt_reset(eng.ctx, self.handle, eng.stream()), "rt_reset")
            return
        slot = check_slot(self.n_streams, stream)
        eng._check(eng.lib.rvcx_rt_reset_stream(eng.ctx, self.handle, slot, eng.stream()), "rt_reset_stream")

    def opts(self, f0_up_key=0, index_rate=0.5, protect=0.5, volume_envelope=1.0, f0_autotune=False,
             f0_autotune_strength=1.0, proposed_pitch=False, proposed_pitch_threshold=155.0,
             gen_precision: str = "fp32", clean_audio=None, clean_strength=None) -> _lib.RtOpts:
        """Per-hop options (rvcx_rt_opts). gen_precision "fp16" runs this hop's generator on fp16 operands (BASELINE
        C5's half precision); the f0 / feature front end, TextEncoder and flow stay fp32-accurate either way.
        clean_audio / clean_strength: None = the group's defaults; a strength outside [0, 1] raises ValueError. They
        are not fields of rvcx_rt_opts (in the reference they are constructor arguments, and the struct keeps its
        layout) but attributes of the returned object, which ``process`` hands to ``rvcx_rt_set_clean`` for the slots
        whose setting changes; an RtOpts without them means the group's defaults."""
        o = _lib.RtOpts()
        self.engine.lib.rvcx_rt_default_opts(ctypes.byref(o))
        # rvc/realtime only retrieves when an index is loaded (pipeline.py:264); index_rate alone does not. The rule is
        # per voice: the rate survives here when any slot's voice has an index, and ``process`` zeroes it for the slots
        # whose voice has none.
        loaded = any(self._has_index(self.voices).values())
        o.f0_up_key, o.index_rate, o.protect = float(f0_up_key), float(index_rate) if loaded else 0.0, float(protect)
        o.volume_envelope, o.f0_autotune = float(volume_envelope), int(bool(f0_autotune))
        o.f0_autotune_strength, o.proposed_pitch = float(f0_autotune_strength), int(bool(proposed_pitch))
        o.proposed_pitch_threshold = float(proposed_pitch_threshold)
        o.gen_precision = {"fp32": 0, "fp16": 1}[gen_precision]
        o.clean_audio = int(self.clean_audio if clean_audio is None else bool(clean_audio))
        o.clean_strength = self.clean_strength if clean_strength is None else check_clean_strength(clean_strength)
        return o

    def _apply_clean(self, opts, active):
        """Bring each active slot's noise gate setting to what its options ask for (no device work)."""
        eng = self.engine
        for b in range(self.n_streams):
            if active is not None and not active[b]:
                continue
            o = opts if isinstance(opts, _lib.RtOpts) else opts[b]
            want = (int(bool(getattr(o, "clean_audio", self.clean_audio))),
                    check_clean_strength(getattr(o, "clean_strength", self.clean_strength)))
            if want != self._clean[b]:
                eng._check(eng.lib.rvcx_rt_set_clean(eng.ctx, self.handle, b, want[0], want[1]), "rt_set_clean")
                self._clean[b] = want

    def process(self, audio_in, opts=None, eps_z=None, eps_src=None, seed: int = 0, active=None):
        """One hop: audio_in [B, block48] @48 kHz (device tensor or numpy) -> (out [B, block48] device tensor,
        vol [B] device tensor). Asynchronous on the current stream.

        opts: one ``RtOpts`` for every stream, or a sequence of B (each stream its own on_request arguments; only
        gen_precision must agree among the active streams). active: a sequence of B booleans, None = all. For an idle
        slot the hop did not happen: its input row is not read, its state is kept, and its out row, vol and SOLA offset
        are zero. eps_z / eps_src rows are indexed by slot. ValueError for a wrong length or mixed gen_precision."""
        eng = self.engine
        t = eng.torch
        opts = self.opts() if opts is None else opts if isinstance(opts, _lib.RtOpts) else list(opts)
        arr, act = hop_arguments(self.n_streams, opts, active)
        if any(o.index_rate > 0 for o in arr):
            # where some of the group's voices have an index and some have none, ``opts`` could not apply the
            # reference's rule (it does not know the slot): it is completed here, per slot. With no index at all a
            # rate set by hand is refused by the library, as before.
            voices = self.voices
            has = self._has_index(voices)
            if any(has.values()) and not all(has.values()):
                zero_rate_without_index(arr, voices, has, act)
        self._apply_clean(opts, act)
        x = eng._dev(audio_in, t.float32).reshape(self.n_streams, self.block_frame)
        ez = eng._opt(eps_z, t.float32)
        es = eng._opt(eps_src, t.float32)
        eng._check(eng.lib.rvcx_rt_process_v(eng.ctx, self.handle, x.data_ptr(), self.sids, arr, act, _ptr(ez),
                                             _ptr(es), eng._seed(seed),
                                             self.out.data_ptr(), self.vol.data_ptr(), self.offs.data_ptr(),
                                             eng.stream()), "rt_process")
        return self.out, self.vol


class VoiceChanger:
    """One realtime stream with the reference's API (rvc/realtime/core.py:329-484).

    ``VoiceChanger(read_chunk_size, cross_fade_overlap_size, extra_convert_size, engine=..., sid=0,
    silent_threshold=0, f0_method="rmvpe", clean_audio=False, clean_strength=0.5)`` then ``on_request(audio_input @48k) -> (audio_out np.float32 [block], vol, [0, ms, 0])``.
    Models come from the Engine (``rvcx.infer.RVCX(...).engine`` or an Engine loaded by hand); an index
    loaded on that Engine (``rvcx.infer.read_index``) is used when index_rate > 0. f0_method is the reference's
    "rmvpe" or "fcpe" (``Engine.load_fcpe``; fcpe_threshold as in StreamGroup); any other name raises ValueError.
    clean_audio / clean_strength are the reference's (core.py:339-350): the noise gate on every hop's model output.
    post_process=True and vad_enabled=True (pedalboard, webrtcvad: CPU libraries outside this path) raise ValueError;
    the reference's remaining keywords are accepted and ignored.
    """

    def __init__(self, read_chunk_size: int, cross_fade_overlap_size: float, extra_convert_size: float,
                 engine: Engine = None, silent_threshold: int = 0, sid: int = 0, f0_method: str = "rmvpe",
                 fcpe_threshold: float = 0.006, clean_audio: bool = False, clean_strength: float = 0.5, **_unused):
        _f0_method_id(f0_method)
        for name in ("post_process", "vad_enabled"):
            if _unused.get(name):
                raise ValueError(f"{name}=True is not supported: this path runs no CPU-side effects or VAD")
        if engine is None:
            raise ValueError("VoiceChanger needs an rvcx Engine with the synthesizer, HuBERT and the f0 method's "
                             "model (RMVPE or FCPE) loaded")
        self.group = StreamGroup(engine, 1, read_chunk_size, cross_fade_overlap_size, extra_convert_size,
                                 silent_threshold, sid, f0_method, fcpe_threshold, clean_audio, clean_strength)
        g = self.group.geometry
        self.block_frame, self.crossfade_frame = g["block48"], g["crossfade48"]
        self.sola_search_frame, self.extra_frame = g["sola_search48"], g["extra48"]
        self.seed = 0

    def process_audio(self, audio_input: np.ndarray, f0_up_key=0, index_rate=0.5, protect=0.5, volume_envelope=1,
                      f0_autotune=False, f0_autotune_strength=1, proposed_pitch=False, proposed_pitch_threshold=155.0,
                      eps_z=None, eps_src=None):
        if audio_input.shape[0] != self.block_frame:
            raise ValueError(f"block must be {self.block_frame} samples (read_chunk_size * 128)")
        o = self.group.opts(f0_up_key, index_rate, protect, volume_envelope, f0_autotune, f0_autotune_strength,
                            proposed_pitch, proposed_pitch_threshold)
        out, vol = self.group.process(np.asarray(audio_input, dtype=np.float32)[None], o, eps_z, eps_src, self.seed)
        self.seed += 1
        out0 = self.group.engine.host(out[0])
        return out0, float(vol[0].item())

    def on_request(self, audio_input: np.ndarray, f0_up_key=0, index_rate=0.5, protect=0.5, volume_envelope=1,
                   f0_autotune=False, f0_autotune_strength=1, proposed_pitch=False, proposed_pitch_threshold=155.0):
        start = time.perf_counter()
        result, vol = self.process_audio(audio_input, f0_up_key, index_rate, protect, volume_envelope, f0_autotune,
                                         f0_autotune_strength, proposed_pitch, proposed_pitch_threshold)
        end = time.perf_counter()
        return result, vol, [0, (end - start) * 1000, 0]

    def close(self):
        self.group.close()
