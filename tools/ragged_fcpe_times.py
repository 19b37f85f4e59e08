"""tools/ragged_batch_times.py's job with FCPE as the pitch network: one FCPE pass per utterance against one ragged
pass per batch, alone and inside the batched pipeline (diagnostic, not product code).

The job: 64 `synthetic.speech_like` utterances, lengths drawn uniformly from 2-30 s at 16 kHz (seed 2024), resident in
HBM; the FCPE model is the 6-layer legacy configuration with seeded weights, as tools/fcpe_times.py loads it. Every
route is timed over the whole job with a host clock around work that ends in a device synchronise, after one untimed
warm-up pass over the same shapes; --reps passes, median reported. Routes timed against each other alternate pass by
pass in the same process. Per bucketing setting, batch in {4, 8, 16} and max_pad in {0.05, 0.125, 0.25}:
  (f) `Engine.fcpe_batch_v` per batch against a loop of `Engine.fcpe` per utterance.
  (g) `Engine.pipeline_batch_v` with f0_method 3 (FCPE per row) and with f0_method 5 (one ragged FCPE pass per batch),
      alternating; the ratio of the medians is called a gain (loss) only if it exceeds the spread of method 3's own
      repeats.
At max_pad 0.125, per batch size: f0_method 0 (RMVPE per row), for the comparison with another build. At the defaults
of convert_many (batch 8, max_pad 0.125): f0_method 5 against f0_method 4 (ragged RMVPE), alternating.
On a library without rvcx_fcpe_batch_v (one built from an older commit through RVCX_LIB) the routes that need it are
skipped: what remains is that commit's f0_method 3 and 0.

    python tools/ragged_fcpe_times.py [--reps 5] [--only BATCH MAX_PAD] > profiles/ragged_fcpe_times.txt

--only times one bucketing setting beside the loop.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import torch  # noqa: E402

from ragged_batch_times import N_UTT, SEED, SR, job_lengths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs=2, metavar=("BATCH", "MAX_PAD"), default=None)
    args = ap.parse_args()
    from rvcx import _lib, offline, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    eng = Engine(0)
    eng.load_synth(normalize_state(synthetic.synth_state(2)), SYNTH_48K_V2)
    eng.load_hubert(normalize_state(synthetic.hubert_state(4)))
    eng.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
    eng.load_fcpe(synthetic.fcpe_state(13, 6, 512), synthetic.fcpe_config(6, 512))
    eng.set_pipeline_highpass()
    ns = job_lengths()
    seconds = sum(ns) / SR
    print(f"library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
    print(f"job: {N_UTT} utterances, seed {SEED}, {min(ns) / SR:.2f} .. {max(ns) / SR:.2f} s, {seconds:.1f} s of audio")
    clips64 = [torch.as_tensor(synthetic.speech_like(n, seed=3000 + i), dtype=torch.float64).to(dev)
               for i, n in enumerate(ns)]
    clips32 = [c.float() for c in clips64]
    order = sorted(range(N_UTT), key=lambda i: -ns[i])
    have_v = "rvcx_fcpe_batch_v" in _lib.exported_symbols()
    if not have_v:
        print("no rvcx_fcpe_batch_v in this library: (f)'s batched half, f0_method 5 and 4 skipped")
    o = {m: eng.pipeline_opts(pitch=2.0, protect=0.33, f0_method=m) for m in ((0, 3, 4, 5) if have_v else (0, 3))}

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
        return out

    res = {}

    def report(name, t, extra=""):
        med = statistics.median(t)
        res[name] = {"s": [round(x, 5) for x in t]}
        print(f"{name:50s} median {med * 1e3:9.2f} ms  min {min(t) * 1e3:9.2f}  max {max(t) * 1e3:9.2f}  "
              f"spread {100 * (max(t) - min(t)) / med:5.2f} %  {seconds / med:9.1f} audio-s/s {extra}", flush=True)
        return med

    def against(name, t_ref, t_new, ref_name):
        mr, mn = statistics.median(t_ref), statistics.median(t_new)
        spread, gain = (max(t_ref) - min(t_ref)) / mr, mr / mn - 1
        word = "gain" if gain > spread else ("loss" if -gain > spread else f"inside {ref_name}'s spread")
        print(f"    {name}: {100 * gain:+.2f} % ({mr / mn:.2f}x; {ref_name}'s own spread {100 * spread:.2f} %): {word}",
              flush=True)

    def fcpe_loop():
        for i in order:
            eng.fcpe(clips32[i])

    def pipe(groups, opts):
        def run():
            for k, g in enumerate(groups):
                eng.pipeline_batch_v([clips64[i] for i in g], opts, seed=k)
        return run

    (t_loop,) = timed(fcpe_loop)
    report("(f) loop of fcpe", t_loop)
    for batch in (4, 8, 16) if args.only is None else (int(args.only[0]),):
        for max_pad in (0.05, 0.125, 0.25) if args.only is None else (float(args.only[1]),):
            groups = offline.bucket(ns, batch, max_pad)
            fr = [n // 160 + 1 for n in ns]
            pad = 1 - sum(fr) / sum(len(g) * max(fr[i] for i in g) for g in groups)
            key = f"batch={batch} max_pad={max_pad}"
            note = f"{len(groups):2d} passes  padded pitch frames {100 * pad:5.2f} %"
            if have_v:
                def fcpe_batched():
                    for g in groups:
                        eng.fcpe_batch_v([clips32[i] for i in g])

                (t_f,) = timed(fcpe_batched)
                report(f"(f) fcpe_batch_v {key}", t_f, note)
                against("(f) against the loop", t_loop, t_f, "the loop")
                t3, t5 = timed(pipe(groups, o[3]), pipe(groups, o[5]))
            else:
                (t3,) = timed(pipe(groups, o[3]))
            report(f"(g) pipeline_batch_v f0_method=3 {key}", t3, note)
            if have_v:
                report(f"(g) pipeline_batch_v f0_method=5 {key}", t5)
                against("(g) method 5 against method 3", t3, t5, "method 3")
            if max_pad == 0.125:
                (t0,) = timed(pipe(groups, o[0]))
                report(f"    pipeline_batch_v f0_method=0 {key}", t0)
            if have_v and (batch, max_pad) == (8, 0.125):
                t4, t5b = timed(pipe(groups, o[4]), pipe(groups, o[5]))
                report(f"    pipeline_batch_v f0_method=4 {key}", t4)
                report(f"    pipeline_batch_v f0_method=5 {key} (again)", t5b)
                against("method 5 against method 4", t4, t5b, "method 4")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
