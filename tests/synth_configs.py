"""The synthesizer configurations beside SYNTH_48K_V2 that the suite runs (test helper, no GPU needed).

    name     upsample_rates   kernels         sr     phone width   source
    v2_40k   10,10,2,2        16,16,4,4       40000  768           the reference's rvc/configs/40000.json
    v2_32k   10,8,2,2         20,16,4,4       32000  768           the reference's rvc/configs/32000.json
    v1_48k   10,6,2,2,2       16,16,4,4,4     48000  256           the list v1 48 kHz checkpoints carry in cpt["config"]
    v1_32k   10,4,2,2,2       16,16,4,4,4     32000  256           the list v1 32 kHz checkpoints carry

What each one reaches that SYNTH_48K_V2 (12,10,2,2 / 24,20,4,4: k = 2u at every stage, polyphase taps 3, pad 1, every
slot of the packed ConvTranspose weight live) does not: v2_40k k = 16, u = 10, p = 3 (of the three packed taps, phases
0..2 and 7..9 have two live, phases 3..6 one, the other slots are zero-filled); v2_32k noise strides 32 / 4 / 2 and upp 320; the v1 lists five stages ending at 16
channels (the generic conv_post, ResBlocks at N = 16) and 256-dim phone features; v1_32k u = 4, k = 16: taps 5, pad 2.
Weights are seeded (rvcx.synthetic.synth_state), nothing is read from a file.
"""
from __future__ import annotations

import dataclasses

from rvcx.config import SYNTH_48K_V2

CONFIGS = {
    "v2_40k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 10, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                                  sr=40000),
    "v2_32k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 8, 2, 2), upsample_kernel_sizes=(20, 16, 4, 4),
                                  sr=32000),
    "v1_48k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 6, 2, 2, 2),
                                  upsample_kernel_sizes=(16, 16, 4, 4, 4), sr=48000, text_enc_hidden_dim=256),
    "v1_32k": dataclasses.replace(SYNTH_48K_V2, upsample_rates=(10, 4, 2, 2, 2),
                                  upsample_kernel_sizes=(16, 16, 4, 4, 4), sr=32000, text_enc_hidden_dim=256),
}
NAMES = tuple(CONFIGS)
SEED_W = 7  # synthetic.synth_state seed of every configuration's weights

_W = {}


def version_of(cfg) -> str:
    """The HuBERT output the configuration's TextEncoder takes: "v1" (final_proj, 256) or "v2" (768)."""
    return "v1" if cfg.text_enc_hidden_dim == 256 else "v2"


def weights_for(name):
    """normalize_state(synthetic.synth_state(SEED_W, cfg)), built once per configuration and never modified."""
    if name not in _W:
        from rvcx import synthetic
        from rvcx.weights import normalize_state

        _W[name] = normalize_state(synthetic.synth_state(SEED_W, CONFIGS[name]))
    return _W[name]


def margin_frames(cfg) -> int:
    """rvcx_dec_margin_frames(cfg): host only, no context and no GPU."""
    import ctypes

    from rvcx import _lib
    from rvcx.engine import Engine

    d = Engine._synth_desc(cfg)
    m = ctypes.c_int32(0)
    rc = _lib.load().rvcx_dec_margin_frames(ctypes.byref(d), ctypes.byref(m))
    assert rc == 0, rc
    return m.value
