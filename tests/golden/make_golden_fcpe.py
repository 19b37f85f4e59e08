"""Generate tests/golden/fcpe_l2.npz by running the REFERENCE's FCPE (survey container only).

Run:  python tests/golden/make_golden_fcpe.py        (needs /root/reference; never on the GPU box)

rvc/lib/predictors/FCPE.py is imported with stubs for what the container lacks and this path never calls
(torchaudio.transforms.Resample, soundfile, local_attention.LocalAttention; librosa with ``filters.mel`` restated in
numpy, as make_golden.py does). It builds FCPE(n_layers=2, n_chans=512), loads rvcx.synthetic.fcpe_state, saves the
checkpoint in the file's own format ({"config", "model"}) to a temporary file and runs FCPEInfer and
FCPEF0Predictor(hop_length=160, sample_rate=16000) from it, in float32 as the reference does.

Per input (speech_like(n, seed=7), n = 15000 / 1000 / 400: 94 frames; 7 frames, reflect padding; 3 frames, the zero
padding branch) it stores the mel, the salience (a forward hook on dense_out, then the sigmoid), the raw f0 at the
threshold (the median of the frame maxima) and compute_f0's interpolated track for p_len = F - 1 (its default), F and
2 F. Weights are NOT stored: tests regenerate them from the seed recorded here.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "fcpe_l2.npz")
sys.path.insert(0, os.path.join(REPO, "retrieval-based-voice-conversion-mlx_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from oracle.rmvpe import mel_filterbank  # noqa: E402
from rvcx import synthetic  # noqa: E402

SEED, N_LAYERS, N_CHANS, AUDIO_SEED = 13, 2, 512, 7
LENGTHS = (15000, 1000, 400)


def install_stubs():
    ta = types.ModuleType("torchaudio")
    tr = types.ModuleType("torchaudio.transforms")
    tr.Resample = None
    ta.transforms = tr
    sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = ta, tr
    sys.modules["soundfile"] = types.ModuleType("soundfile")
    la = types.ModuleType("local_attention")
    la.LocalAttention = None
    sys.modules["local_attention"] = la
    lib = types.ModuleType("librosa")
    filters = types.ModuleType("librosa.filters")

    def mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, **kw):
        return mel_filterbank(sr, n_fft, n_mels, fmin, fmax if fmax is not None else sr / 2.0, htk)

    filters.mel = mel
    lib.filters = filters
    sys.modules["librosa"], sys.modules["librosa.filters"] = lib, filters


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from rvc.lib.predictors import FCPE as ref

    torch.manual_seed(0)
    cfg = synthetic.fcpe_config(N_LAYERS, N_CHANS)
    net = ref.FCPE(input_channel=128, out_dims=360, n_layers=N_LAYERS, n_chans=N_CHANS)
    sd = {k: torch.from_numpy(v) for k, v in synthetic.fcpe_state(SEED, N_LAYERS, N_CHANS).items()}
    want = net.state_dict()
    assert set(sd) == set(want), (sorted(set(want) - set(sd)), sorted(set(sd) - set(want)))
    for k, v in want.items():
        assert tuple(v.shape) == tuple(sd[k].shape), (k, v.shape, sd[k].shape)
    out = {"seed": SEED, "n_layers": N_LAYERS, "n_chans": N_CHANS, "audio_seed": AUDIO_SEED,
           "lengths": np.asarray(LENGTHS)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fcpe.pt")
        torch.save({"config": cfg, "model": sd}, path)
        pred = ref.FCPEF0Predictor(path, hop_length=160, dtype=torch.float32, device="cpu", sample_rate=16000)
    infer = pred.fcpe
    hooked = []
    infer.model.dense_out.register_forward_hook(lambda m, i, o: hooked.append(torch.sigmoid(o.detach())[0]))
    for n in LENGTHS:
        audio = synthetic.speech_like(n, seed=AUDIO_SEED).astype(np.float32)
        x = torch.from_numpy(audio)
        mel = infer.wav2mel(audio=x[None, :], sample_rate=16000)[0]
        hooked.clear()
        infer(x, sr=16000, threshold=0.0)
        sal = hooked[0].numpy()
        thr = float(np.median(sal.max(1)))
        f0 = infer(x, sr=16000, threshold=thr)[0, :, 0].numpy()
        f0_arg = infer.model(mel=mel[None], infer=True, return_hz_f0=True, cdecoder="argmax")[0, :, 0].detach().numpy()
        F = sal.shape[0]
        assert mel.shape == (F, 128) and f0.shape == (F,) and F == n // 160 + 1
        pred.threshold = thr
        out.update({f"mel_{n}": mel.numpy(), f"sal_{n}": sal, f"thr_{n}": np.float64(thr), f"f0_{n}": f0,
                    f"f0_argmax_{n}": f0_arg})
        for p_len in (F - 1, F, 2 * F):
            out[f"interp_{n}_{p_len}"] = np.asarray(pred.compute_f0(audio, p_len), np.float64)
        print(n, "frames", F, "thr", thr, "voiced", float((f0 > 0).mean()), "peaks", len(np.unique(sal.argmax(1))))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
