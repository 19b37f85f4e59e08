"""Device time of a realtime hop with f0_method "rmvpe" and "fcpe", and of the batched FCPE forward beside the loop it
replaces (diagnostic, not product code).

B = 16 streams at the C5 geometry (read_chunk_size 96: 256 ms hops, 13920-sample convert buffers), seeded weights, the
legacy FCPE configuration (6 layers, 512 channels). HIP events around R back-to-back calls after a warm-up; the two
variants of a comparison alternate within the run, `rounds` times, and the mean per call of every round is kept:
the figures printed are the mean over the rounds and their lowest and highest value (the spread).

  hop_rmvpe / hop_fcpe   one rvcx_rt_process hop for the 16 streams (everything of the hop, not the f0 stage alone)
  fcpe_batch             one rvcx_fcpe_b call on the 16 convert buffers
  fcpe_loop              16 back-to-back rvcx_fcpe calls on the same buffers (outputs preallocated; the host issues
                         16 x the launches, so this figure includes whatever of that the device has to wait for)

    python tools/stream_f0_times.py [--reps 20] [--rounds 5]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from rvcx import synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    eng = Engine(0)
    eng.load_synth(normalize_state(synthetic.synth_state(2)), SYNTH_48K_V2)
    eng.load_hubert(normalize_state(synthetic.hubert_state(4)))
    eng.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
    eng.load_fcpe(synthetic.fcpe_state(13, 6, 512), synthetic.fcpe_config(6, 512))
    geom = dict(read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5, silent_threshold=-90.0)
    groups = {m: StreamGroup(eng, B, f0_method=m, fcpe_threshold=0.5, **geom) for m in ("rmvpe", "fcpe")}
    blk, n = groups["fcpe"].geometry["block48"], groups["fcpe"].geometry["convert16"]
    hops = 4  # distinct input blocks, cycled
    x48 = torch.as_tensor(np.stack([synthetic.speech_like(blk * hops, seed=300 + s, sr=48000) for s in range(B)]),
                          dtype=torch.float32).to(dev)
    conv = torch.as_tensor(np.stack([synthetic.speech_like(n, seed=500 + s) for s in range(B)]),
                           dtype=torch.float32).to(dev)
    F = n // 160 + 1
    f0 = torch.empty((B, F), dtype=torch.float64, device=dev)
    fo = ctypes.c_int64(0)
    count = {"hop": 0}

    def hop(m):
        g = groups[m]
        h = count["hop"] % hops
        count["hop"] += 1
        g.process(x48[:, h * blk:(h + 1) * blk], opts[m], seed=count["hop"])

    def fcpe_loop():
        for b in range(B):
            eng._check(eng.lib.rvcx_fcpe(eng.ctx, conv[b].data_ptr(), n, 0.5, 0, 0, 0, f0[b].data_ptr(), None, F,
                                         ctypes.byref(fo), eng.stream()), "fcpe")

    def fcpe_batch():
        eng._check(eng.lib.rvcx_fcpe_b(eng.ctx, conv.data_ptr(), n, n, B, 0.5, 0, f0.data_ptr(), None, eng.stream()),
                   "fcpe_b")

    opts = {m: g.opts(index_rate=0.0) for m, g in groups.items()}
    stages = {"hop_rmvpe": lambda: hop("rmvpe"), "hop_fcpe": lambda: hop("fcpe"), "fcpe_batch": fcpe_batch,
              "fcpe_loop": fcpe_loop}
    for fn in stages.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    per_round = {k: [] for k in stages}
    for _ in range(args.rounds):
        for name, fn in stages.items():  # the variants alternate within every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize(dev)
            per_round[name].append(a.elapsed_time(b) / args.reps)
    eng.check_device_status()
    res = {}
    for name, v in per_round.items():
        res[name] = {"mean_ms": round(float(np.mean(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        print(f"{name:12s} mean {res[name]['mean_ms']:8.4f} ms  (rounds {min(v):.4f} .. {max(v):.4f})", flush=True)
    print(json.dumps({"streams": B, "convert16": n, "frames": F, "reps": args.reps, "rounds": args.rounds,
                      "fcpe_layers": 6, "ms": res,
                      "hop_fcpe_over_rmvpe": round(res["hop_fcpe"]["mean_ms"] / res["hop_rmvpe"]["mean_ms"], 3),
                      "loop_over_batch": round(res["fcpe_loop"]["mean_ms"] / res["fcpe_batch"]["mean_ms"], 2)}))
    for g in groups.values():
        g.close()
    eng.close()


if __name__ == "__main__":
    main()
