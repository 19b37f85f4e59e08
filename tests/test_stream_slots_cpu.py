"""Host-only checks of the per-slot stream interface: the two entry points (rvcx_rt_process_v, rvcx_rt_reset_stream)
are exported with the argument types include/rvcx.h declares, rvcx_rt_opts keeps its layout, and StreamGroup's
argument checks (rvcx.realtime.hop_arguments / check_slot) raise ValueError without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_exported_with_declared_types():
    from rvcx import _lib

    lib = _lib.load()
    assert {"rvcx_rt_process_v", "rvcx_rt_reset_stream"} <= set(_lib.EXPORTS)
    assert {"rvcx_rt_process_v", "rvcx_rt_reset_stream"} <= set(_lib.exported_symbols())
    vp, P = ctypes.c_void_p, ctypes.POINTER
    # (ctx, rt, d_in, sids, opts, active, d_eps_z, d_eps_src, seed, d_out, d_vol, d_offs, stream)
    assert lib.rvcx_rt_process_v.argtypes == [vp, vp, vp, P(ctypes.c_int32), P(_lib.RtOpts), P(ctypes.c_uint8), vp, vp,
                                              ctypes.c_uint64, vp, vp, vp, vp]
    assert lib.rvcx_rt_process_v.restype is ctypes.c_int
    # (ctx, rt, stream_index, stream)
    assert lib.rvcx_rt_reset_stream.argtypes == [vp, vp, ctypes.c_int, vp]
    assert lib.rvcx_rt_reset_stream.restype is ctypes.c_int
    # the old entry point keeps its prototype
    assert lib.rvcx_rt_process.argtypes == [vp, vp, vp, P(ctypes.c_int32), P(_lib.RtOpts), vp, vp, ctypes.c_uint64, vp,
                                            vp, vp, vp]
    # null arguments are refused before any device is touched
    assert lib.rvcx_rt_process_v(None, None, None, None, None, None, None, None, 0, None, None, None, None) != 0
    assert lib.rvcx_rt_reset_stream(None, None, 0, None) != 0


def test_header_declares_what_the_binding_calls():
    with open(os.path.join(ROOT, "include", "rvcx.h")) as f:
        h = re.sub(r"\s+", " ", f.read())
    assert ("int rvcx_rt_process_v(rvcx_ctx* ctx, rvcx_rt* rt, const float* d_in, const int32_t* sids, "
            "const rvcx_rt_opts* opts, const uint8_t* active, const float* d_eps_z, const float* d_eps_src, "
            "uint64_t seed, float* d_out, float* d_vol, int32_t* d_offs, void* stream);") in h
    assert "int rvcx_rt_reset_stream(rvcx_ctx* ctx, rvcx_rt* rt, int stream_index, void* stream);" in h


def test_rt_opts_layout_unchanged():
    from rvcx import _lib

    o = _lib.RtOpts
    assert ctypes.sizeof(o) == 72
    assert [(n, getattr(o, n).offset) for n, _ in o._fields_] == [
        ("f0_up_key", 0), ("index_rate", 8), ("protect", 16), ("volume_envelope", 24), ("f0_autotune", 32),
        ("f0_autotune_strength", 40), ("proposed_pitch", 48), ("proposed_pitch_threshold", 56), ("gen_precision", 64)]
    # the library fills the same 72 bytes: a guard word after the struct survives rvcx_rt_default_opts
    buf = (ctypes.c_uint8 * 80)(*([0xAB] * 80))
    assert _lib.load().rvcx_rt_default_opts(ctypes.cast(buf, ctypes.POINTER(o))) == 0
    assert bytes(buf[72:]) == b"\xab" * 8
    d = ctypes.cast(buf, ctypes.POINTER(o)).contents
    assert (d.protect, d.volume_envelope, d.f0_autotune_strength, d.gen_precision) == (0.5, 1.0, 1.0, 0)
    assert ctypes.sizeof(_lib.RtDesc) == 40


def _opts(**kw):
    from rvcx import _lib

    o = _lib.RtOpts()
    assert _lib.load().rvcx_rt_default_opts(ctypes.byref(o)) == 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_hop_arguments_validation():
    from rvcx import _lib
    from rvcx.realtime import check_slot, hop_arguments

    a, b = _opts(f0_up_key=12.0), _opts(f0_up_key=-5.0, f0_autotune=1)
    arr, act = hop_arguments(3, a)
    assert act is None and len(arr) == 3 and [o.f0_up_key for o in arr] == [12.0] * 3
    arr, act = hop_arguments(2, [a, b], [True, 0])
    assert [o.f0_up_key for o in arr] == [12.0, -5.0] and arr[1].f0_autotune == 1 and list(act) == [1, 0]
    arr[0].f0_up_key = 1.0  # a copy: the caller's struct is not aliased
    assert a.f0_up_key == 12.0
    with pytest.raises(ValueError):
        hop_arguments(3, [a, b])
    with pytest.raises(ValueError):
        hop_arguments(2, [a, b, a])
    with pytest.raises(ValueError):
        hop_arguments(2, [a, b], [True])
    with pytest.raises(ValueError):
        hop_arguments(2, [a, 3.0])
    lowp = _opts(gen_precision=1)
    with pytest.raises(ValueError):
        hop_arguments(2, [a, lowp])
    with pytest.raises(ValueError):
        hop_arguments(3, [a, lowp, a], [True, True, False])
    hop_arguments(2, [a, lowp], [True, False])  # an idle slot's precision does not count
    hop_arguments(2, [lowp, lowp])
    hop_arguments(2, [a, lowp], [False, False])
    assert check_slot(4, 3) == 3 and check_slot(4, 0) == 0
    for bad in (4, -1, 1.5, True):
        with pytest.raises(ValueError):
            check_slot(4, bad)
    assert isinstance(arr, ctypes.Array) and arr._type_ is _lib.RtOpts


def test_stream_group_signature():
    import inspect

    from rvcx.realtime import StreamGroup, VoiceChanger

    p = inspect.signature(StreamGroup.process).parameters
    assert list(p)[:6] == ["self", "audio_in", "opts", "eps_z", "eps_src", "seed"] and p["active"].default is None
    assert inspect.signature(StreamGroup.reset).parameters["stream"].default is None
    assert "active" not in inspect.signature(VoiceChanger.on_request).parameters
