"""Streaming fixture with f0_method "fcpe" from the REFERENCE's own realtime code (survey container only).

Run:  python tests/golden/make_golden_stream_fcpe.py      (needs /root/reference; never on the GPU box)

As make_golden_stream.py (whose stubs, inputs and noise scheme are imported), for 4 independent streams x 4 hops at
the C5 geometry with ``VoiceChanger(96, 0.1, 0.5, ..., f0_method="fcpe", silent_threshold=-90, sid=s % 4)``; stream
3's hops 1-2 are digital silence (the gated path).

The reference's FCPE class (rvc/lib/predictors/f0.py:59-89) calls ``torchfcpe.spawn_infer_model_from_pt`` with the
package's bundled model. torchfcpe is not installed and its bundled model is not readable here, so that one function
is replaced by an ADAPTER -- the one piece of this path that is not the reference's code: its ``.infer(x [1, n], sr,
decoder_mode, threshold)`` asserts decoder_mode == "local_argmax" and sr == 16000 and calls the reference's own
``FCPEInfer`` (rvc/lib/predictors/FCPE.py:726-764), built from the seeded 2-layer, 512-channel checkpoint of
fcpe_l2.npz exactly as make_golden_fcpe.py builds it. get_f0's call, the realtime quantisation, the pitch buffers
and everything after are the reference's.

Threshold. The reference passes FCPE's 0.006, which means nothing for seeded weights (every frame would be voiced).
A first run records each hop's salience (a forward hook on dense_out) on the convert buffers, which do not depend on
the threshold. Of every frame maximum over all streams and hops the sorted values between the 30th and 70th
percentile are taken; the threshold is the midpoint of the widest gap between two consecutive ones. The adapter
passes it instead of 0.006 in the second run, the one that is stored.

Margins. With tests/fcpe_ref.py and tests/parity_anchor.py the float64 salience of every recorded convert buffer and
its fp32 gap are computed; `gap` is the largest. Asserted: every frame maximum lies at least 2 K gaps (K = 8) from the
threshold. The device is within K gaps of float64 and the reference's fp32 run within one, so no voicing decision can
differ. A voiced frame is "unsure" when its float64 peak leads the best bin more than 4 bins away by less than 2 K
gaps: the peak could then move outside the +-4 local_argmax window (inside it, a flip barely moves the weighted
mean). A hop is flagged when its buffer holds such a frame. Asserted: at most 25 % of the ungated hops are flagged;
INPUT_SEED0 steps through INPUT_SEEDS until that holds.

Saved (tests/golden/stream_fcpe_4.npz): out16 (fp16), vol, sola_offset, the threshold, the gap, the per-hop unsure
flags, the float64 frame maxima, the input and noise seeds and the inputs' SHA-256. Weights are not stored.
"""
from __future__ import annotations

import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_stream as ms  # noqa: E402  (stubs, digest; make_golden's paths and weight builders)

mg = ms.mg

import torch  # noqa: E402

N_STREAMS, HOPS, BLOCK = 4, 4, 96 * 128
INPUT_SEEDS = (400, 420, 440, 460, 480)  # tried in order until at most 25 % of the ungated hops are unsure
NOISE_SEED0 = 900
SILENT_STREAM, SILENT_HOPS = 3, (1, 2)
FCPE_SEED, FCPE_LAYERS, FCPE_CHANS = 13, 2, 512  # the model of fcpe_l2.npz
OPTS = dict(ms.OPTS)
K = 8


def stream_inputs(seed0):
    from rvcx import synthetic

    x = np.stack([synthetic.speech_like(BLOCK * HOPS, seed=seed0 + s, sr=48000).astype(np.float32)
                  for s in range(N_STREAMS)])
    x[SILENT_STREAM, SILENT_HOPS[0] * BLOCK:(SILENT_HOPS[-1] + 1) * BLOCK] = 0.0
    return x


class TorchFcpeAdapter:
    """Stands in for the object torchfcpe.spawn_infer_model_from_pt returns: NOT the reference's code."""

    def __init__(self, fcpe_infer):
        self.fcpe = fcpe_infer
        self.threshold = None  # None: pass the caller's
        self.buffers, self.salience = [], []
        fcpe_infer.model.dense_out.register_forward_hook(
            lambda m, i, o: self.salience.append(torch.sigmoid(o.detach())[0].numpy().copy()))

    def infer(self, x, sr, decoder_mode, threshold):
        assert decoder_mode == "local_argmax" and sr == 16000, (decoder_mode, sr)
        assert x.dim() == 2 and x.shape[0] == 1 and x.dtype == torch.float32
        self.buffers.append(x[0].numpy().copy())
        return self.fcpe(x[0], sr=sr, threshold=threshold if self.threshold is None else self.threshold)


def pick_threshold(mx):
    """The midpoint of the widest gap between consecutive sorted frame maxima within [30th, 70th] percentile."""
    v = np.sort(np.asarray(mx, np.float64).reshape(-1))
    lo, hi = np.percentile(v, 30), np.percentile(v, 70)
    v = v[(v >= lo) & (v <= hi)]
    i = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[i] + v[i + 1]))


def margins(buffers, thr):
    """Per buffer: float64 frame maxima [F], fp32 gap, unsure-frame mask [F] (see the module docstring, gap given
    later). Returns (mx64 [N][F], gap, lead [N][F]) with lead = peak - best bin more than 4 bins away."""
    import fcpe_ref as fr
    import parity_anchor as pa
    from rvcx import synthetic
    from rvcx.weights import check_fcpe_state, fcpe_sizes

    cfg = synthetic.fcpe_config(FCPE_LAYERS, FCPE_CHANS)
    w = check_fcpe_state(synthetic.fcpe_state(FCPE_SEED, FCPE_LAYERS, FCPE_CHANS), cfg)
    z = fcpe_sizes(cfg)
    mx, lead, gap = [], [], 0.0
    bins = np.arange(360)
    for a in buffers:
        t = torch.from_numpy(a)
        ref64, g = pa.anchor(lambda dt, t=t: fr.salience_from_audio(pa.weights(w, dt), z, t.to(dt)))["out"]
        gap = max(gap, g)
        pk = ref64.argmax(1)
        far = np.abs(bins[None, :] - pk[:, None]) > 4
        mx.append(ref64.max(1))
        lead.append(ref64.max(1) - np.where(far, ref64, -np.inf).max(1))
    return np.stack(mx), gap, np.stack(lead)


def run_streams(core, model_path, x, adapter, record):
    outs = np.zeros((N_STREAMS, HOPS, BLOCK), np.float32)
    vols = np.zeros((N_STREAMS, HOPS), np.float64)
    offs = np.full((N_STREAMS, HOPS), -1, np.int64)
    orig_randn, orig_argmax = torch.randn_like, torch.argmax
    for s in range(N_STREAMS):
        vc = core.VoiceChanger(96, 0.1, 0.5, model_path=model_path, index_path="", f0_method="fcpe",
                               silent_threshold=-90, sid=s % 4)
        rt = vc.vc_model
        assert (rt.convert_feature_size_16k, rt.skip_head, rt.return_length, rt.convert_buffer.shape[0]) == \
            (87, 50, 37, 13920)
        ns = mg.NoiseStream(NOISE_SEED0 + s)
        seen = []

        def argmax(t, *a, **k):
            r = orig_argmax(t, *a, **k)
            if t.dim() == 1 and t.shape[0] == vc.sola_search_frame + 1:
                seen.append(int(r))
            return r

        torch.randn_like, torch.argmax = ns, argmax
        try:
            for h in range(HOPS):
                res, vol, _ = vc.on_request(x[s, h * BLOCK:(h + 1) * BLOCK].copy(), **OPTS)
                outs[s, h], vols[s, h], offs[s, h] = res, vol, seen[-1]
        finally:
            torch.randn_like, torch.argmax = orig_randn, orig_argmax
        assert len(ns.draws) == 2 * HOPS and len(seen) == HOPS
        if record:
            print(f"stream {s}: offs {offs[s].tolist()} vol {np.round(vols[s], 4).tolist()}", flush=True)
    assert len(adapter.buffers) == len(adapter.salience) == N_STREAMS * HOPS
    return outs, vols, offs


def main():
    from transformers import HubertConfig, HubertModel  # noqa: F401  (resolve before the module stubs exist)

    ms.install_realtime_stubs()
    la = types.ModuleType("local_attention")
    la.LocalAttention = None
    sys.modules["local_attention"] = la
    sys.path.insert(0, mg.REF)
    scratch = tempfile.mkdtemp(prefix="rvc_stream_fcpe_golden_")
    os.makedirs(os.path.join(scratch, "rvc", "models", "predictors"))
    shutil.copytree(os.path.join(mg.REF, "rvc", "configs"), os.path.join(scratch, "rvc", "configs"),
                    ignore=shutil.ignore_patterns("*.py", "__pycache__"))
    os.chdir(scratch)
    torch.manual_seed(0)
    torch.set_num_threads(8)

    from rvcx import synthetic
    from rvcx.config import SYNTH_48K_V2

    sd = mg.to_torch_state(synthetic.synth_state(mg.SEEDS["synth"]))
    model_path = os.path.join(scratch, "model.pth")
    torch.save({"config": SYNTH_48K_V2.as_list(), "weight": sd, "f0": 1, "version": "v2", "vocoder": "HiFi-GAN",
                "sr": 48000}, model_path)
    hub = mg.build_hubert()

    from rvc.lib.predictors import FCPE as ref_fcpe

    fcpe_path = os.path.join(scratch, "fcpe_seeded.pt")
    torch.save({"config": synthetic.fcpe_config(FCPE_LAYERS, FCPE_CHANS),
                "model": {k: torch.from_numpy(v)
                          for k, v in synthetic.fcpe_state(FCPE_SEED, FCPE_LAYERS, FCPE_CHANS).items()}}, fcpe_path)
    adapter = TorchFcpeAdapter(ref_fcpe.FCPEInfer(fcpe_path, device="cpu", dtype=torch.float32))

    import rvc.lib.predictors.f0 as ref_f0
    import rvc.realtime.pipeline as rtp
    from rvc.realtime import core

    ref_f0.spawn_infer_model_from_pt = lambda *a, **k: adapter
    rtp.load_embedding = lambda *a, **k: hub  # never download

    for seed0 in INPUT_SEEDS:
        x = stream_inputs(seed0)
        # run 1: the convert buffers and their salience (independent of the threshold)
        adapter.threshold, adapter.buffers, adapter.salience = None, [], []
        _, vols1, _ = run_streams(core, model_path, x, adapter, record=False)
        buffers = [b.copy() for b in adapter.buffers]
        thr = pick_threshold(np.stack(adapter.salience).max(2))
        mx64, gap, lead = margins(buffers, thr)
        dist = np.abs(mx64 - thr)
        print(f"seed0 {seed0}: threshold {thr:.6f} gap {gap:.3e} min |max - thr| {dist.min():.3e} "
              f"(needs {2 * K * gap:.3e}) voiced share {float((mx64 > thr).mean()):.3f}", flush=True)
        assert dist.min() >= 2 * K * gap, "a frame maximum lies within 2 K gaps of the threshold"
        unsure = ((mx64 > thr) & (lead < 2 * K * gap)).any(1).reshape(N_STREAMS, HOPS)
        ungated = vols1 > 0
        share = float((unsure & ungated).sum()) / float(ungated.sum())
        print(f"seed0 {seed0}: unsure hops {int((unsure & ungated).sum())} of {int(ungated.sum())} ungated", flush=True)
        if share <= 0.25:
            break
    else:
        raise AssertionError("no input seed of INPUT_SEEDS keeps the unsure hops within 25 %")
    # run 2: the stored one, at the chosen threshold
    adapter.threshold, adapter.buffers, adapter.salience = thr, [], []
    outs, vols, offs = run_streams(core, model_path, x, adapter, record=True)
    for a, b in zip(buffers, adapter.buffers):
        assert np.array_equal(a, b)
    assert np.array_equal(vols, vols1)
    # the audio buffer keeps 1600 samples of the hop before, so the first silent hop still has a volume; the second is
    # digital silence throughout: vol 0, the gated path
    assert vols[SILENT_STREAM, SILENT_HOPS[-1]] == 0 and (np.delete(vols, SILENT_STREAM, 0) > 0).all()
    out = os.path.join(mg.OUT, "stream_fcpe_4.npz")
    np.savez_compressed(out, out16=outs.astype(np.float16), vol=vols, sola_offset=offs, n_streams=N_STREAMS, hops=HOPS,
                        block=BLOCK, input_seed0=seed0, noise_seed0=NOISE_SEED0, silent_stream=SILENT_STREAM,
                        silent_hops=np.asarray(SILENT_HOPS), sids=np.arange(N_STREAMS) % 4,
                        f0_up_key=OPTS["f0_up_key"], protect=OPTS["protect"], input_sha256=ms.inputs_digest(x),
                        threshold=np.float64(thr), gap=np.float64(gap), unsure=unsure,
                        frame_max64=mx64.reshape(N_STREAMS, HOPS, -1), fcpe_seed=FCPE_SEED, fcpe_layers=FCPE_LAYERS,
                        fcpe_chans=FCPE_CHANS)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
