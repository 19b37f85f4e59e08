"""A folder-like job of utterances of different lengths: one pass per utterance against batched passes over rows of
similar length, for the whole pipeline and for HuBERT alone (diagnostic, not product code).

The job: 64 `synthetic.speech_like` utterances, lengths drawn uniformly from 2-30 s at 16 kHz (one seed, printed),
resident in HBM. Every route is timed over the whole job with a host clock around work that ends in a device
synchronise, after one untimed warm-up pass over the same shapes; --reps passes, median reported:
  (a) loop of `Engine.pipeline_ex` per utterance, longest first: the only route for such a job before
      rvcx_pipeline_batch_v. Its own min .. max over the repeats is the spread every comparison is held against.
  (b) `Engine.pipeline_batch_v` per batch of `offline.bucket(lengths, batch, max_pad)`, batch in {4, 8, 16} and
      max_pad in {0.05, 0.125, 0.25}, with the share of computed synthesizer frames that are padding.
  (c) `Engine.hubert_batch_v` over the same batches against a loop of `Engine.hubert`.
  (d) (b) with f0_method 4: the rows of a batch in one ragged RMVPE pass instead of one pass per row. (b) and (d) of a
      setting are timed alternately, pass by pass, in the same process; the ratio of their medians is printed and
      called a gain (loss) only if it exceeds the spread of (b)'s own repeats.
  (e) `Engine.rmvpe_batch_v` over the same batches against a loop of `Engine.rmvpe`.
A batched setting is called faster (slower) only if its median lies below (above) the loop's own min .. max.
(d) and (e) are skipped on a library without rvcx_rmvpe_batch_v (one built from an older commit through RVCX_LIB).

    python tools/ragged_batch_times.py [--reps 5] [--loop-only] [--only BATCH MAX_PAD] > profiles/ragged_batch_times.txt

--loop-only times the two loops alone. It calls nothing the ragged entry points added, so with RVCX_LIB pointing at a
library built from an older commit it measures that commit's route. --only times one batched setting beside the loops.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED, N_UTT, SR = 2024, 64, 16000


def job_lengths():
    rng = np.random.Generator(np.random.PCG64(SEED))
    return [int(n) for n in rng.integers(2 * SR, 30 * SR + 1, size=N_UTT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--only", nargs=2, metavar=("BATCH", "MAX_PAD"), default=None)
    args = ap.parse_args()
    from rvcx import _lib, offline, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine, hubert_frames
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    eng = Engine(0)
    eng.load_synth(normalize_state(synthetic.synth_state(2)), SYNTH_48K_V2)
    eng.load_hubert(normalize_state(synthetic.hubert_state(4)))
    eng.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
    eng.set_pipeline_highpass()
    opts = eng.pipeline_opts(pitch=2.0, protect=0.33)
    ns = job_lengths()
    seconds = sum(ns) / SR
    print(f"library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
    print(f"job: {N_UTT} utterances, seed {SEED}, {min(ns) / SR:.2f} .. {max(ns) / SR:.2f} s, {seconds:.1f} s of audio")
    clips64 = [torch.as_tensor(synthetic.speech_like(n, seed=3000 + i), dtype=torch.float64).to(dev)
               for i, n in enumerate(ns)]
    clips32 = [c.float() for c in clips64]
    order = sorted(range(N_UTT), key=lambda i: -ns[i])

    def once(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def timed(*fns):
        """Each fn warmed up once (every shape of the timed pass), then --reps passes of each, alternating."""
        for fn in fns:
            fn()
        out = [[] for _ in fns]
        for _ in range(args.reps):
            for k, fn in enumerate(fns):
                out[k].append(once(fn))
        return out[0] if len(fns) == 1 else out

    have_v = "rvcx_rmvpe_batch_v" in _lib.exported_symbols()
    if not have_v:
        print("no rvcx_rmvpe_batch_v in this library: (d) and (e) skipped")
    opts4 = eng.pipeline_opts(pitch=2.0, protect=0.33, f0_method=4)

    res = {}

    def report(name, t, ref=None, extra=""):
        med = statistics.median(t)
        verdict = ""
        if ref is not None:
            verdict = "faster" if med < min(ref) else ("slower" if med > max(ref) else "inside the loop's spread")
        res[name] = {"s": [round(x, 5) for x in t], "audio_s_per_s": round(seconds / med, 1)}
        print(f"{name:44s} median {med * 1e3:9.2f} ms  min {min(t) * 1e3:9.2f}  max {max(t) * 1e3:9.2f}  "
              f"{seconds / med:9.1f} audio-s/s {extra} {verdict}", flush=True)

    def pipe_loop():
        for i in order:
            eng.pipeline_ex(clips64[i], opts, seed=i)

    def hub_loop():
        for i in order:
            eng.hubert(clips32[i])

    t_pipe = timed(pipe_loop)
    report("(a) loop of pipeline_ex", t_pipe,
           extra=f"(spread {100 * (max(t_pipe) - min(t_pipe)) / statistics.median(t_pipe):.1f} %)")
    t_hub = timed(hub_loop)
    report("(c) loop of hubert", t_hub, extra=f"(spread {100 * (max(t_hub) - min(t_hub)) / statistics.median(t_hub):.1f} %)")

    def rm_loop():
        for i in order:
            eng.rmvpe(clips32[i])

    t_rm = timed(rm_loop)
    report("(e) loop of rmvpe", t_rm, extra=f"(spread {100 * (max(t_rm) - min(t_rm)) / statistics.median(t_rm):.1f} %)")
    if not args.loop_only:
        frames = [eng.pipeline_frames(n, opts) for n in ns]
        for batch in (4, 8, 16) if args.only is None else (int(args.only[0]),):
            for max_pad in (0.05, 0.125, 0.25) if args.only is None else (float(args.only[1]),):
                groups = offline.bucket(ns, batch, max_pad)
                pad = 1 - sum(frames) / sum(len(g) * frames[g[0]] for g in groups)
                hpad = 1 - sum(hubert_frames(n) for n in ns) / sum(len(g) * hubert_frames(ns[g[0]]) for g in groups)
                key = f"batch={batch} max_pad={max_pad}"

                def pipe_batched():
                    for k, g in enumerate(groups):
                        eng.pipeline_batch_v([clips64[i] for i in g], opts, seed=k)

                def hub_batched():
                    for g in groups:
                        eng.hubert_batch_v([clips32[i] for i in g])

                def pipe_batched4():
                    for k, g in enumerate(groups):
                        eng.pipeline_batch_v([clips64[i] for i in g], opts4, seed=k)

                def rm_batched():
                    for g in groups:
                        eng.rmvpe_batch_v([clips32[i] for i in g])

                t_b, t_d = timed(pipe_batched, pipe_batched4) if have_v else (timed(pipe_batched), None)
                report(f"(b) pipeline_batch_v {key}", t_b, t_pipe,
                       f"{len(groups):2d} passes  padded frames {100 * pad:5.2f} %")
                res[f"(b) pipeline_batch_v {key}"].update(passes=len(groups), pad_share=round(pad, 4))
                if have_v:
                    report(f"(d) pipeline_batch_v f0_method=4 {key}", t_d, t_pipe)
                    mb, md = statistics.median(t_b), statistics.median(t_d)
                    spread = (max(t_b) - min(t_b)) / mb
                    gain = mb / md - 1
                    word = "gain" if gain > spread else ("loss" if -gain > spread else "inside (b)'s spread")
                    print(f"    (d) against (b): {100 * gain:+.2f} % ((b)'s own spread {100 * spread:.2f} %): {word}",
                          flush=True)
                    res[f"(d) pipeline_batch_v f0_method=4 {key}"].update(gain_over_b=round(gain, 4),
                                                                          b_spread=round(spread, 4))
                report(f"(c) hubert_batch_v {key}", timed(hub_batched), t_hub,
                       f"{len(groups):2d} passes  padded frames {100 * hpad:5.2f} %")
                if have_v:
                    report(f"(e) rmvpe_batch_v {key}", timed(rm_batched), t_rm, f"{len(groups):2d} passes")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
