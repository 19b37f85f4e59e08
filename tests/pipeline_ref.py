"""The oracle pipeline with recorded noise, for the tests that hold the device pipeline to it."""
import numpy as np
import torch

class NoiseRecorder:
    """noise_fn for OraclePipeline: seeded draws, kept in call order for the device run."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.z, self.src = [], []

    def __call__(self, shape, which):
        a = self.rng.standard_normal(shape).astype(np.float32)
        (self.z if which == "z" else self.src).append(a.reshape(-1))
        return torch.from_numpy(a)

    def cat(self):
        return np.concatenate(self.z), np.concatenate(self.src)


def oracle_pipeline(synth_w, hubert_w, rmvpe_w, noise, **cfg):
    from oracle.pipeline import OraclePipeline
    from rvcx.config import HUBERT_BASE, RMVPE_CFG, SYNTH_48K_V2

    return OraclePipeline(48000, synth_w=synth_w, synth_cfg=SYNTH_48K_V2, hubert_w=hubert_w, hubert_cfg=HUBERT_BASE,
                          rmvpe_w=rmvpe_w, rmvpe_cfg=RMVPE_CFG, noise_fn=noise, **cfg)
