"""sha256 of the raw output bytes of every model entry point on the seeded synthetic models (diagnostic, not product
code): run it on two builds and diff the outputs to show that a host-side refactor left every result bit-identical.

One line per output: RMVPE (single and batched, a frame count that is no multiple of 32), the FCPE mel and salience
(a normal length, and one shorter than the window: zero padding and the duplicated last frame), HuBERT, CREPE, the
synthesizer with each vocoder, a 6-hop stream group (once more with a volume envelope on one of its streams), both
pipeline forms for f0_method 0 / 2 / 3 under autotune and under proposed pitch and with a volume envelope, the batched
pipeline's salience, and the ragged forms: HuBERT over rows of five lengths, the pipeline over rows of three lengths
(plain and with a volume envelope) and over two equal rows, RMVPE over rows of five lengths in one ragged pass and the
ragged pipeline with it (f0_method 4). Then, as plain integers, Engine.workspace_bytes of five calls: the arena query
runs the pipelines in their sizing form. Last, FCPE over rows of five lengths in one ragged pass, the ragged pipeline
with it (f0_method 5) and its arena query, and the strided copy-out of equal rows: HuBERT, RMVPE and FCPE over equal
rows whose output rows the caller spaces wider than the pass writes them.

    python tools/output_digests.py > digests.txt
"""
import ctypes
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def show(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(f"{name:36s} {h.hexdigest()}", flush=True)


def synth_inputs(cfg, B, T, seed):
    from rvcx import synthetic

    rng = np.random.Generator(np.random.PCG64(seed))
    phone = rng.standard_normal((B, T, cfg.text_enc_hidden_dim)).astype(np.float32)
    pitch = rng.integers(1, 256, size=(B, T)).astype(np.int64)
    return phone, [T] * B, pitch, synthetic.f0_walk(B, T, seed=seed + 1), list(range(B))


def strided_v(eng, entry, audios, F, nb, *mode):
    """rvcx_rmvpe_batch_v / rvcx_fcpe_batch_v itself on equal rows, the f0 rows F + 5 and the salience rows F + 3 frames
    apart (as run_rows_c of the ragged tests calls them): the rows' own frames of both outputs."""
    t = eng.torch
    a = eng._dev(np.stack(audios), t.float32)
    B, n = a.shape
    f0 = t.zeros((B, F + 5), dtype=t.float64, device=eng.device)
    sal = t.zeros((B, F + 3, nb), dtype=t.float32, device=eng.device)
    F_arr = (ctypes.c_int64 * B)()
    eng._check(getattr(eng.lib, entry)(eng.ctx, a.data_ptr(), (ctypes.c_int64 * B)(*[n] * B), n, B, 0.03, *mode,
                                       f0.data_ptr(), F + 5, F_arr, sal.data_ptr(), F + 3, eng.stream()), entry)
    assert [int(v) for v in F_arr] == [F] * B
    return f0[:, :F], sal[:, :F]


def main():
    from rvcx import _lib, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup
    from rvcx.weights import normalize_state

    f32 = np.float32
    eng = Engine(0)
    eng.load_synth(normalize_state(synthetic.synth_state(2)), SYNTH_48K_V2)
    eng.load_hubert(normalize_state(synthetic.hubert_state(4)))
    eng.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
    eng.load_crepe(synthetic.crepe_state("tiny"))
    eng.load_fcpe(synthetic.fcpe_state(13, 2, 512), synthetic.fcpe_config(2, 512))

    a = synthetic.speech_like(10000, seed=21).astype(f32)  # 63 frames
    show("rmvpe B=1", *eng.rmvpe(a, want_hidden=True))
    show("rmvpe_batch B=2", *eng.rmvpe_batch(np.stack([a, 0.5 * a[::-1]]), want_hidden=True))
    for n in (8000, 400):  # 400 < win: zero padding, 2 STFT frames of 3
        x = synthetic.speech_like(n, seed=22).astype(f32)
        show(f"fcpe_mel n={n}", eng.fcpe_mel(x))
        show(f"fcpe n={n}", *eng.fcpe(x, want_salience=True))
    show("fcpe_batch B=2", *eng.fcpe_batch(np.stack([a, 0.5 * a[::-1]]), want_salience=True))
    show("hubert", eng.hubert(a))
    show("crepe", *eng.crepe(a, want_periodicity=True, want_probs=True))
    show("crepe rvc", *eng.crepe(a, want_probs=True, semantics="rvc"))

    show("synth_infer HiFi-GAN", eng.synth_infer(*synth_inputs(SYNTH_48K_V2, 2, 40, 31), seed=7))
    for voc in ("MRF HiFi-GAN", "RefineGAN"):
        cfg = dataclasses.replace(SYNTH_48K_V2, vocoder=voc)
        e2 = Engine(0)
        e2.load_synth(normalize_state(synthetic.synth_state(2, cfg)), cfg)
        show(f"synth_infer {voc}", e2.synth_infer(*synth_inputs(cfg, 2, 40, 31), seed=7))
        e2.close()

    B, hops = 2, 6
    grp = StreamGroup(eng, B, read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5,
                      silent_threshold=-90.0, sid=list(range(B)))
    block = grp.geometry["block48"]
    audio = np.stack([synthetic.speech_like(block * hops, seed=60 + b, sr=48000).astype(f32) for b in range(B)])
    outs = [grp.process(audio[:, h * block:(h + 1) * block], grp.opts(index_rate=0.0), seed=h)[0].clone()
            for h in range(hops)]
    show(f"stream group B={B} {hops} hops", *outs)
    per_stream = [grp.opts(index_rate=0.0), grp.opts(index_rate=0.0, volume_envelope=0.4)]
    outs = [grp.process(audio[:, h * block:(h + 1) * block], per_stream, seed=h)[0].clone() for h in range(hops)]
    show(f"stream group B={B} envelope on 1", *outs)
    grp.close()
    show("hubert_batch_v 5 rows", *eng.hubert_batch_v([synthetic.speech_like(n, seed=70 + i).astype(f32) for i, n in
                                                       enumerate((40000, 400, 21000, 20700, 16000))]))

    eng.set_pipeline_highpass()
    speech = synthetic.speech_like(24000, seed=7)
    two = np.stack([speech, 0.7 * np.roll(speech, 4000)])
    for method in (0, 2, 3):
        for adj in ({"f0_autotune": 1}, {"proposed_pitch": 1}):
            opts = eng.pipeline_opts(f0_method=method, pitch=2.0, **adj)
            tag = f"f0_method={method} {next(iter(adj))}"
            show(f"pipeline_ex {tag}", *eng.pipeline_ex(speech, opts, seed=3, want_f0=True))
            show(f"pipeline_batch {tag}", *eng.pipeline_batch(two, opts, sids=[0, 1], seed=3, want_f0=True))
    env = eng.pipeline_opts(pitch=2.0, volume_envelope=0.5)
    show("pipeline_ex envelope", *eng.pipeline_ex(speech, env, seed=3, want_f0=True))
    show("pipeline_batch envelope", *eng.pipeline_batch(two, env, sids=[0, 1], seed=3, want_f0=True))
    show("pipeline_batch want_hidden", *eng.pipeline_batch(two, eng.pipeline_opts(pitch=2.0), sids=[0, 1], seed=3,
                                                           want_f0=True, want_hidden=True))
    ys, f0s = eng.pipeline_batch_v(list(two), env, sids=[0, 1], seed=3, want_f0=True)
    show("pipeline_batch_v equal rows envelope", *ys, *f0s)
    ragged = [synthetic.speech_like(n, seed=90 + b) for b, n in enumerate((24000, 40000, 8000, 24000))]
    for tag, kw in (("plain", {}), ("envelope", {"volume_envelope": 0.5})):
        opts = eng.pipeline_opts(pitch=2.0, t_pad=4800, t_pad_tgt=14400, **kw)
        ys, f0s = eng.pipeline_batch_v(ragged, opts, sids=[0, 3, 7, 0], seed=3, want_f0=True)
        show(f"pipeline_batch_v ragged {tag}", *ys, *f0s)
    if "rvcx_rmvpe_batch_v" in _lib.exported_symbols():  # a library from before the ragged RMVPE pass ends here
        rows = [synthetic.speech_like(n, seed=70 + i).astype(f32) for i, n in
                enumerate((2720, 4960, 5280, 10080, 16000))]
        f0s, hids = eng.rmvpe_batch_v(rows, want_hidden=True)
        show("rmvpe_batch_v 5 rows", *f0s, *hids)
        opts = eng.pipeline_opts(pitch=2.0, t_pad=4800, t_pad_tgt=14400, f0_method=4)
        ys, f0s = eng.pipeline_batch_v(ragged, opts, sids=[0, 3, 7, 0], seed=3, want_f0=True)
        show("pipeline_batch_v ragged f0_method=4", *ys, *f0s)
        ragged_kw = {"t_pad": 4800, "t_pad_tgt": 14400}
        for B, n, kw in ((1, 24000, {}), (1, 24000, {"f0_method": 3}),
                         (1, 128000, {"t_max": 48000, "t_center": 32000, "t_query": 8000}),
                         (4, 40000, ragged_kw), (4, 40000, {**ragged_kw, "f0_method": 4})):
            tag = "".join(f" {k}={v}" for k, v in kw.items())
            need = eng.workspace_bytes(n, B=B, opts=eng.pipeline_opts(**kw))
            print(f"workspace_bytes B={B} n={n}{tag}: {need}", flush=True)
    if "rvcx_fcpe_batch_v" in _lib.exported_symbols():  # a library from before the ragged FCPE pass ends here
        rows = [synthetic.speech_like(n, seed=70 + i).astype(f32) for i, n in
                enumerate((1000, 2400, 13920, 20480, 48000))]
        f0s, sals = eng.fcpe_batch_v(rows, want_salience=True)
        show("fcpe_batch_v 5 rows", *f0s, *sals)
        kw = {"t_pad": 4800, "t_pad_tgt": 14400, "f0_method": 5}
        ys, f0s = eng.pipeline_batch_v(ragged, eng.pipeline_opts(pitch=2.0, **kw), sids=[0, 3, 7, 0], seed=3, want_f0=True)
        show("pipeline_batch_v ragged f0_method=5", *ys, *f0s)
        need = eng.workspace_bytes(40000, B=4, opts=eng.pipeline_opts(**kw))
        print(f"workspace_bytes B=4 n=40000{''.join(f' {k}={v}' for k, v in kw.items())}: {need}", flush=True)
        eq = [synthetic.speech_like(5280, seed=80 + b).astype(f32) for b in range(3)]
        show("hubert_batch_v equal rows strided", *eng.hubert_batch_v(eq[:2], ld_rows=16 + 3))
        show("rmvpe_batch_v equal rows strided", *strided_v(eng, "rvcx_rmvpe_batch_v", eq, 34, 360))
        show("fcpe_batch_v equal rows strided", *strided_v(eng, "rvcx_fcpe_batch_v", eq, 34, 360, 0))
    eng.close()


if __name__ == "__main__":
    main()
