"""The streaming oracle with f0_method "fcpe" (test helper, no GPU needed): oracle.realtime.OracleVoiceChanger whose
get_f0 takes the raw local_argmax track from the FCPE restatement (tests/fcpe_ref.py) instead of RMVPE -- rvc/realtime/
pipeline.py:148-155, where FCPE.get_f0 returns the network's track as it is (F = n // 160 + 1 frames, zeros where
unvoiced, no interpolation). A second yardstick for the device's "fcpe" streams beside the reference run of
tests/golden/make_golden_stream_fcpe.py: it shares no code with that script's torchfcpe adapter."""
import numpy as np
import torch

import fcpe_ref as fr
from oracle.realtime import OracleVoiceChanger, circular_write


class FcpeOracleVoiceChanger(OracleVoiceChanger):
    def __init__(self, synth_w, synth_cfg, hubert_w, hubert_cfg, fcpe_w, fcpe_sizes, fcpe_threshold=0.006, **kw):
        """fcpe_w: rvcx.weights.check_fcpe_state's dict as float32 torch tensors; fcpe_sizes: rvcx.weights.fcpe_sizes."""
        super().__init__(synth_w, synth_cfg, hubert_w, hubert_cfg, None, None, **kw)
        self.fw, self.fz, self.fcpe_threshold = fcpe_w, fcpe_sizes, float(fcpe_threshold)
        assert self.fz["sampling_rate"] == 16000 and self.fz["hop_size"] == 160

    def get_f0(self, x, pitch, pitchf, f0_up_key=0, f0_autotune=False, f0_autotune_strength=1.0,
               proposed_pitch=False, proposed_pitch_threshold=155.0):
        assert not f0_autotune and not proposed_pitch, "the plain shift is all this helper restates"
        sal = fr.salience_from_audio(self.fw, self.fz, x.float())
        f0 = fr.decode(sal, self.fw["cent_table"], self.fcpe_threshold).float().numpy()
        f0 *= pow(2, f0_up_key / 12)
        f0 = torch.from_numpy(f0).float()
        f0_mel = 1127.0 * torch.log(1.0 + f0 / 700.0)  # the realtime quantisation (pipeline.py:196-203)
        f0_mel = torch.clip((f0_mel - 50.0) * 254 / (1100.0 - 50.0) + 1, 1, 255, out=f0_mel)
        f0_coarse = torch.round(f0_mel, out=f0_mel).long()
        circular_write(f0_coarse, pitch)
        circular_write(f0, pitchf)
        return pitch.unsqueeze(0), pitchf.unsqueeze(0)


def stream_inputs(g):
    from rvcx import synthetic

    S, H, blk = int(g["n_streams"]), int(g["hops"]), int(g["block"])
    x = np.stack([synthetic.speech_like(blk * H, seed=int(g["input_seed0"]) + s, sr=48000).astype(np.float32)
                  for s in range(S)])
    hops = [int(h) for h in g["silent_hops"]]
    x[int(g["silent_stream"]), hops[0] * blk:(hops[-1] + 1) * blk] = 0.0
    return x


def hop_noise(rngs, I, T, upp):
    """The fixture's recorded noise for one hop: per stream PCG64 draws, eps_z then eps_src (make_golden.NoiseStream)."""
    S = len(rngs)
    ez = np.empty((S, I, T), np.float32)
    es = np.empty((S, T * upp), np.float32)
    for s in range(S):
        ez[s] = rngs[s].standard_normal((1, I, T)).astype(np.float32)[0]
        es[s] = rngs[s].standard_normal((1, T * upp, 1)).astype(np.float32).reshape(-1)
    return ez, es
