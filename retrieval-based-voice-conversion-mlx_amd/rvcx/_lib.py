"""ctypes binding of librvcx.so: the product C-ABI declared in include/rvcx.h (SIG) and the kernel-level test
entries declared in include/rvcx_test.h (TEST_SIG).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, importing
the compute path raises ``RvcxLibraryError``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVCX_LIB", os.path.join(_HERE, "librvcx.so"))

RVCX_MODEL_SYNTH, RVCX_MODEL_HUBERT, RVCX_MODEL_RMVPE, RVCX_MODEL_CREPE, RVCX_MODEL_FCPE = 0, 1, 2, 3, 4

STATUS = {
    0: "RVCX_OK", -1: "RVCX_E_INVALID", -2: "RVCX_E_SHAPE", -3: "RVCX_E_HIP", -4: "RVCX_E_OOM",
    -5: "RVCX_E_STATE", -6: "RVCX_E_CAPACITY",
}


class RvcxLibraryError(ImportError):
    pass


class RvcxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class SynthDesc(ctypes.Structure):
    _fields_ = [
        ("inter_channels", ctypes.c_int), ("hidden_channels", ctypes.c_int), ("filter_channels", ctypes.c_int),
        ("n_heads", ctypes.c_int), ("n_layers", ctypes.c_int), ("kernel_size", ctypes.c_int),
        ("n_resblocks", ctypes.c_int), ("resblock_kernel_sizes", ctypes.c_int * 4),
        ("resblock_dilation_sizes", (ctypes.c_int * 4) * 4), ("n_dilations", ctypes.c_int),
        ("n_upsample", ctypes.c_int), ("upsample_rates", ctypes.c_int * 8),
        ("upsample_initial_channel", ctypes.c_int), ("upsample_kernel_sizes", ctypes.c_int * 8),
        ("spk_embed_dim", ctypes.c_int), ("gin_channels", ctypes.c_int), ("sr", ctypes.c_int),
        ("text_enc_hidden_dim", ctypes.c_int), ("no_f0", ctypes.c_int), ("vocoder", ctypes.c_int),
    ]


VOCODERS = {"HiFi-GAN": 0, "MRF HiFi-GAN": 1, "RefineGAN": 2}


class VoiceDesc(ctypes.Structure):
    """rvcx_voice_desc (include/rvcx.h)."""
    _fields_ = [("synth", SynthDesc), ("config_set", ctypes.c_int), ("ready", ctypes.c_int),
                ("index_d", ctypes.c_int64), ("index_ntotal", ctypes.c_int64), ("index_nlist", ctypes.c_int64),
                ("index_nprobe", ctypes.c_int64), ("weight_bytes", ctypes.c_int64), ("split_bytes", ctypes.c_int64)]


class PipelineOpts(ctypes.Structure):
    """rvcx_pipeline_opts (include/rvcx.h)."""
    _fields_ = [
        ("sid", ctypes.c_int), ("version", ctypes.c_int), ("pitch", ctypes.c_double), ("protect", ctypes.c_float),
        ("rmvpe_threshold", ctypes.c_float), ("t_pad", ctypes.c_int64), ("t_pad_tgt", ctypes.c_int64),
        ("t_query", ctypes.c_int64), ("t_center", ctypes.c_int64), ("t_max", ctypes.c_int64),
        ("f0_autotune", ctypes.c_int), ("f0_autotune_strength", ctypes.c_double), ("proposed_pitch", ctypes.c_int),
        ("proposed_pitch_threshold", ctypes.c_double), ("volume_envelope", ctypes.c_double),
        ("mlx_semantics", ctypes.c_int), ("index_rate", ctypes.c_double), ("f0_method", ctypes.c_int),
        ("fcpe_threshold", ctypes.c_float),
    ]


class FcpeDesc(ctypes.Structure):
    """rvcx_fcpe_desc (include/rvcx.h)."""
    _fields_ = [("sampling_rate", ctypes.c_int), ("n_fft", ctypes.c_int), ("win_size", ctypes.c_int),
                ("hop_size", ctypes.c_int), ("num_mels", ctypes.c_int), ("fmin", ctypes.c_float),
                ("fmax", ctypes.c_float), ("n_layers", ctypes.c_int), ("n_chans", ctypes.c_int),
                ("out_dims", ctypes.c_int)]


class RtDesc(ctypes.Structure):
    """rvcx_rt_desc (include/rvcx.h)."""
    _fields_ = [("n_streams", ctypes.c_int), ("read_chunk_size", ctypes.c_int),
                ("cross_fade_overlap_size", ctypes.c_double), ("extra_convert_size", ctypes.c_double),
                ("silent_threshold", ctypes.c_double), ("f0_method", ctypes.c_int),
                ("fcpe_threshold", ctypes.c_float)]


class RtOpts(ctypes.Structure):
    """rvcx_rt_opts (include/rvcx.h)."""
    _fields_ = [("f0_up_key", ctypes.c_double), ("index_rate", ctypes.c_double), ("protect", ctypes.c_float),
                ("volume_envelope", ctypes.c_double), ("f0_autotune", ctypes.c_int),
                ("f0_autotune_strength", ctypes.c_double), ("proposed_pitch", ctypes.c_int),
                ("proposed_pitch_threshold", ctypes.c_double), ("gen_precision", ctypes.c_int)]


class ConvTestDesc(ctypes.Structure):
    """rvcx_conv_test_desc (include/rvcx_test.h): one 1-D contraction as the dispatcher's record takes it."""
    _fields_ = [
        ("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p),
        ("mask", ctypes.c_void_p), ("pre_mask", ctypes.c_void_p), ("y", ctypes.c_void_p),
        ("T_in", ctypes.c_int), ("C_in", ctypes.c_int), ("N", ctypes.c_int), ("taps", ctypes.c_int),
        ("dil", ctypes.c_int), ("pad", ctypes.c_int), ("stride", ctypes.c_int), ("T_out", ctypes.c_int),
        ("ldx", ctypes.c_int), ("ldy", ctypes.c_int), ("ldr", ctypes.c_int),
        ("batch", ctypes.c_int),
        ("x_bs", ctypes.c_int64), ("y_bs", ctypes.c_int64), ("res_bs", ctypes.c_int64), ("mask_bs", ctypes.c_int64),
        ("pre_mask_bs", ctypes.c_int64),
        ("batch_inner", ctypes.c_int),
        ("x_bs2", ctypes.c_int64), ("w_bs2", ctypes.c_int64), ("y_bs2", ctypes.c_int64), ("res_bs2", ctypes.c_int64),
        ("bias_bs2", ctypes.c_int64),
        ("pre_act", ctypes.c_int), ("pre_slope", ctypes.c_float),
        ("act", ctypes.c_int), ("slope", ctypes.c_float), ("alpha", ctypes.c_float),
        ("res_mode", ctypes.c_int), ("acc_mode", ctypes.c_int), ("acc_div", ctypes.c_float),
        ("gate_h", ctypes.c_int), ("gate_g", ctypes.c_void_p), ("gate_g_bs", ctypes.c_int64),
        ("ln_g", ctypes.c_void_p), ("ln_b", ctypes.c_void_p), ("ln_eps", ctypes.c_float),
        ("nz_har", ctypes.c_void_p), ("nz_bs", ctypes.c_int64),
        ("nz_stride", ctypes.c_int), ("nz_kk", ctypes.c_int), ("nz_u", ctypes.c_int), ("nz_C", ctypes.c_int),
        ("nz_w", ctypes.c_void_p), ("nz_b", ctypes.c_void_p),
        ("route", ctypes.c_int), ("no_splitk", ctypes.c_int),
    ]


class ConvPlanForm(ctypes.Structure):
    """rvcx_conv_plan_form (include/rvcx_test.h): the record's fields a 1-D ConvTestDesc lacks."""
    _fields_ = [("W_in", ctypes.c_int), ("W_out", ctypes.c_int), ("KH", ctypes.c_int), ("KW", ctypes.c_int),
                ("padh", ctypes.c_int), ("padw", ctypes.c_int), ("out_map", ctypes.c_int), ("out_cv", ctypes.c_int),
                ("lowp", ctypes.c_int), ("ldw", ctypes.c_int), ("w_ts", ctypes.c_int64),
                ("w_bs", ctypes.c_int64), ("bias_bs", ctypes.c_int64)]


class IndexBuildOpts(ctypes.Structure):
    """rvcx_index_build_opts (include/rvcx.h)."""
    _fields_ = [("niter", ctypes.c_int), ("nprobe", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("init_rows", ctypes.POINTER(ctypes.c_int64))]


vp, i64, i32, f32, f64, u64 = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double,
                               ctypes.c_uint64)
P = ctypes.POINTER

# symbol -> (restype, argtypes): each entry point is listed once, under the header that declares it
# (tests/test_abi_cpu.py holds both tables against the headers, name by name and parameter count by parameter count)

# the product ABI (include/rvcx.h)
SIG = {
    "rvcx_create": (i32, [P(vp), i32]),
    "rvcx_destroy": (i32, [vp]),
    "rvcx_last_error": (ctypes.c_char_p, [vp]),
    "rvcx_set_synth_config": (i32, [vp, P(SynthDesc)]),
    "rvcx_upload": (i32, [vp, i32, ctypes.c_char_p, vp, P(i64), i32]),
    "rvcx_finalize": (i32, [vp, i32]),
    "rvcx_hubert": (i32, [vp, vp, i64, i32, vp, i64, P(i64), vp]),
    "rvcx_rmvpe": (i32, [vp, vp, i64, f32, vp, i64, P(i64), vp, vp]),
    "rvcx_f0_post": (i32, [vp, vp, i64, f64, vp, vp, vp, vp]),
    "rvcx_synth_infer": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp]),
    "rvcx_synth_infer_ex": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, f64, vp, vp, u64, vp, vp, vp, vp, vp, P(i32),
                                  vp]),
    "rvcx_dec_only": (i32, [vp, i32, i32, vp, vp, vp, vp, u64, vp, vp]),
    "rvcx_voice_conversion": (i32, [vp, vp, i64, vp, vp, i32, f32, f64, vp, vp, u64, vp, i64, P(i64), vp]),
    "rvcx_synth_upp": (i32, [vp]),
    "rvcx_set_highpass": (i32, [vp, vp, vp, vp, i32]),
    "rvcx_profile": (i32, [vp, i32]),
    "rvcx_profile_read": (i32, [vp, P(f64), P(f64), P(i64)]),
    "rvcx_profile_read_ex": (i32, [vp, P(f64), P(f64), P(i64), P(f64)]),
    "rvcx_pipeline": (i32, [vp, vp, i64, i32, f64, f32, i64, i64, vp, vp, u64, vp, i64, P(i64), vp, vp]),
    "rvcx_pipeline_default_opts": (i32, [P(PipelineOpts)]),
    "rvcx_pipeline_ex": (i32, [vp, vp, i64, P(PipelineOpts), vp, vp, u64, vp, i64, P(i64), vp, vp]),
    "rvcx_f0_autotune": (i32, [vp, vp, i64, f64, i32, vp]),
    "rvcx_rmvpe_decode": (i32, [vp, vp, i64, f32, vp, vp]),
    "rvcx_crepe": (i32, [vp, vp, i64, f32, f32, f32, vp, vp, vp, i64, P(i64), vp]),
    "rvcx_crepe_ex": (i32, [vp, vp, i64, f32, f32, f32, i32, vp, vp, vp, vp, i64, P(i64), vp]),
    "rvcx_crepe_decode": (i32, [vp, vp, i64, f32, f32, f32, i32, vp, vp, vp, vp]),
    "rvcx_set_fcpe_config": (i32, [vp, P(FcpeDesc)]),
    "rvcx_fcpe": (i32, [vp, vp, i64, f32, i32, i32, i64, vp, vp, i64, P(i64), vp]),
    "rvcx_fcpe_decode": (i32, [vp, vp, i64, f32, i32, i32, i64, vp, vp]),
    "rvcx_fcpe_b": (i32, [vp, vp, i64, i64, i32, f32, i32, vp, vp, vp]),
    "rvcx_split_audio": (i32, [vp, vp, i64, i32, f64, i32, P(i64), i64, P(i64), vp]),
    "rvcx_index_load": (i32, [vp, vp, i64]),
    "rvcx_index_unload": (i32, [vp]),
    "rvcx_index_info": (i32, [vp, P(i64), P(i64), P(i64), P(i64)]),
    "rvcx_index_set_nprobe": (i32, [vp, i64]),
    "rvcx_index_search": (i32, [vp, vp, i64, i32, vp, vp, vp]),
    "rvcx_index_reconstruct_n": (i32, [vp, i64, i64, vp, vp]),
    "rvcx_index_retrieve": (i32, [vp, vp, i64, i32, f64, vp, vp]),
    "rvcx_index_default_build_opts": (i32, [P(IndexBuildOpts)]),
    "rvcx_index_build": (i32, [vp, vp, i64, i32, i64, P(IndexBuildOpts), vp]),
    "rvcx_index_centroids": (i32, [vp, vp, vp]),
    "rvcx_index_save": (i32, [vp, vp, i64, P(i64)]),
    "rvcx_pipeline_batch": (i32, [vp, vp, i64, i64, i32, P(PipelineOpts), P(ctypes.c_int32), vp, vp, u64, vp, i64,
                                  P(i64), vp, vp, vp]),
    "rvcx_pipeline_batch_v": (i32, [vp, vp, P(i64), i64, i32, P(PipelineOpts), P(ctypes.c_int32), vp, vp, u64, vp,
                                    i64, P(i64), vp, i64, vp]),
    "rvcx_set_highpass_sos": (i32, [vp, vp, i32]),
    "rvcx_workspace_bytes": (i32, [vp, i32, i64, P(PipelineOpts), P(i64), vp]),
    "rvcx_set_workspace": (i32, [vp, vp, i64]),
    "rvcx_workspace_info": (i32, [vp, P(i64), P(i64), P(i64)]),
    "rvcx_highpass_pad": (i32, [vp, vp, i64, i64, vp, vp, vp]),
    "rvcx_resample_poly_len": (i32, [i64, i32, i32, P(i64)]),
    "rvcx_resample_poly_v": (i32, [vp, vp, i32, i32, P(i64), i64, i32, i32, i32, vp, i64, vp, i64, P(i64), vp]),
    "rvcx_hubert_batch": (i32, [vp, vp, i64, i64, i32, i32, vp, i64, P(i64), vp]),
    "rvcx_hubert_batch_v": (i32, [vp, vp, P(i64), i64, i32, i32, vp, i64, P(i64), vp]),
    "rvcx_rmvpe_batch": (i32, [vp, vp, i64, i64, i32, f32, vp, i64, P(i64), vp, vp]),
    "rvcx_rmvpe_batch_v": (i32, [vp, vp, P(i64), i64, i32, f32, vp, i64, P(i64), vp, i64, vp]),
    "rvcx_fcpe_batch_v": (i32, [vp, vp, P(i64), i64, i32, f32, i32, vp, i64, P(i64), vp, i64, vp]),
    "rvcx_rt_default_desc": (i32, [P(RtDesc)]),
    "rvcx_rt_default_opts": (i32, [P(RtOpts)]),
    "rvcx_rt_create": (i32, [vp, P(RtDesc), P(vp)]),
    "rvcx_rt_destroy": (i32, [vp, vp]),
    "rvcx_rt_geometry": (i32, [vp, P(i64)]),
    "rvcx_rt_reset": (i32, [vp, vp, vp]),
    "rvcx_rt_process": (i32, [vp, vp, vp, P(ctypes.c_int32), P(RtOpts), vp, vp, u64, vp, vp, vp, vp]),
    "rvcx_rt_process_v": (i32, [vp, vp, vp, P(ctypes.c_int32), P(RtOpts), P(ctypes.c_uint8), vp, vp, u64, vp, vp,
                                vp, vp]),
    "rvcx_rt_reset_stream": (i32, [vp, vp, i32, vp]),
    "rvcx_spectral_gate": (i32, [vp, vp, i32, i64, i64, i32, P(f32), vp, i64, vp, vp]),
    "rvcx_rt_set_clean": (i32, [vp, vp, i32, i32, f64]),
    "rvcx_device_status": (i32, [vp, vp]),
    "rvcx_index_parse": (i32, [vp, i64, P(i64), P(i64), P(i64), P(i64), ctypes.c_char_p, i64]),
    "rvcx_config_info": (i32, [vp, vp, i64, P(i64)]),
    "rvcx_profile_read_kinds": (i32, [vp, P(f64), P(f64), P(i64), P(f64), i32, P(f64), P(f64), P(f64), P(f64),
                                      P(i64)]),
    "rvcx_profile_kind_name": (ctypes.c_char_p, [i32]),
    "rvcx_pipeline_batch_voices": (i32, [vp, vp, P(i64), i64, i32, P(PipelineOpts), P(ctypes.c_int32),
                                         P(ctypes.c_int32), vp, vp, u64, vp, i64, P(i64), vp, i64, vp]),
    "rvcx_voice_new": (i32, [vp, P(i32)]),
    "rvcx_voice_select": (i32, [vp, i32]),
    "rvcx_voice_current": (i32, [vp, P(i32)]),
    "rvcx_voice_info": (i32, [vp, i32, P(VoiceDesc)]),
    "rvcx_voice_free": (i32, [vp, i32]),
    "rvcx_rt_set_voice": (i32, [vp, vp, i32, i32]),
    "rvcx_rt_get_voices": (i32, [vp, P(ctypes.c_int32)]),
}

# kernel-level entry points for the numerics tests (include/rvcx_test.h): exported, not part of the product ABI
TEST_SIG = {
    "rvcx_set_conv_math": (i32, [vp, i32]),
    "rvcx_conv1d": (i32, [vp, vp, i64, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, i64, vp]),
    "rvcx_conv1d_gen": (i32, [vp, vp, i64, i32, vp, vp, i32, i32, i32, i32, i32, f32, i32, f32, vp, i32, f32, i32,
                              vp, vp]),
    "rvcx_conv1d_ex": (i32, [vp, P(ConvTestDesc), P(i32), P(i32), vp]),
    "rvcx_conv2d3x3": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
    "rvcx_convtranspose2d_s2": (i32, [vp, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
    "rvcx_conv2d3x3_v": (i32, [vp, vp, i32, P(i32), i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
    "rvcx_convtranspose2d_s2_v": (i32, [vp, vp, i32, P(i32), i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
    "rvcx_flash_attention": (i32, [vp, vp, i32, i32, i32, i32, f32, vp, vp, i32, vp, vp, vp]),
    "rvcx_resblock_pair": (i32, [vp, vp, i32, i64, i32, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp]),
    "rvcx_performer_attention": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, vp, vp]),
    "rvcx_performer_attention_b": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    "rvcx_performer_attention_v": (i32, [vp, vp, vp, vp, i32, i32, P(i32), i32, vp, i32, vp, vp]),
    "rvcx_fcpe_mel": (i32, [vp, vp, i64, vp, i64, P(i64), vp]),
    "rvcx_set_dec_window": (i32, [vp, i32]),
    "rvcx_dec_margin_frames": (i32, [P(SynthDesc), P(i32)]),
    "rvcx_conv_plan": (i32, [P(ConvTestDesc), P(ConvPlanForm), i32, i32, i32, i32, i32, i32, P(i32), P(i32), P(i32),
                             P(i32)]),
    "rvcx_kmeans_assign": (i32, [vp, vp, i64, i32, vp, i64, vp, vp, vp]),
    "rvcx_kmeans_update": (i32, [vp, vp, i64, i32, vp, i64, vp, vp, vp]),
    "rvcx_rt_model_rows": (i32, [vp, vp, i32, vp, i64, vp]),
    "rvcx_gru_bidir": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
    "rvcx_gru_bidir_v": (i32, [vp, vp, i32, P(i32), vp, vp, vp, vp, vp, i64, vp]),
    "rvcx_dec_source": (i32, [vp, i32, i32, vp, vp, u64, vp, vp]),
    "rvcx_rg_resample_dw": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, vp, i32, vp]),
    "rvcx_rg_lerp_up_cat": (i32, [vp, vp, i32, i32, i32, i32, i32, f32, vp, i32, vp, i32, vp]),
    "rvcx_rg_adain": (i32, [vp, vp, i32, i32, i32, vp, vp, u64, f32, vp, i32, f32, vp]),
}

EXPORTS = list(SIG)
TEST_EXPORTS = list(TEST_SIG)

_lib: Optional[ctypes.CDLL] = None


def load(path: Optional[str] = None) -> ctypes.CDLL:
    """Load librvcx.so and declare every prototype. Raises RvcxLibraryError when absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RvcxLibraryError(f"librvcx.so not found at {p}; build it with __graft_entry__.build() "
                               "(make -C retrieval-based-voice-conversion-mlx_amd/csrc)")
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:
        raise RvcxLibraryError(f"cannot load {p}: {e}") from e
    for name, (res, args) in {**SIG, **TEST_SIG}.items():
        if not hasattr(lib, name):  # reported by exported_symbols(); an older build lacks newer entry points
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def exported_symbols(path: Optional[str] = None):
    """Names of the C-ABI entry points that resolve in the library (no compute call)."""
    lib = load(path)
    return [n for n in EXPORTS + TEST_EXPORTS if hasattr(lib, n)]


def index_parse(data: bytes) -> dict:
    """Validate a faiss IndexIVFFlat file image on the host (rvcx_index_parse; no context, no GPU).
    Returns dict(d, ntotal, nlist, nprobe); raises RvcxError for anything the loader would refuse."""
    lib = load()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    v = [ctypes.c_int64(0) for _ in range(4)]
    err = ctypes.create_string_buffer(512)
    rc = lib.rvcx_index_parse(buf, len(data), *[ctypes.byref(x) for x in v], err, 512)
    if rc != 0:
        raise RvcxError(rc, err.value.decode(errors="replace"))
    return dict(zip(("d", "ntotal", "nlist", "nprobe"), (x.value for x in v)))
