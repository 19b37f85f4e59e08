"""Device time of the FCPE pitch network on the C2 clip (diagnostic, not product code).

rvcx_fcpe with the legacy configuration (6 layers, 512 channels, seeded weights) on the 216100-sample C2 clip, beside
RMVPE on the same clip from the same run, and the Performer attention kernels alone at that length (8 heads x 1351
frames, one layer's call: pass A, the slab combine and pass B). HIP events around R back-to-back calls after a
warm-up; every figure is the mean per call.

    python tools/fcpe_times.py [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from rvcx import synthetic
    from rvcx.engine import Engine
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    eng = Engine(0)
    eng.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
    cfg = synthetic.fcpe_config(6, 512)
    eng.load_fcpe(synthetic.fcpe_state(13, 6, 512), cfg)
    n = 216100
    audio = torch.as_tensor(synthetic.speech_like(n, seed=1000), dtype=torch.float32).to(dev)
    F = n // 160 + 1
    rng = np.random.Generator(np.random.PCG64(3))
    q, k, v = (torch.as_tensor(rng.standard_normal((8, F, 64)).astype(np.float32), device=dev) for _ in range(3))
    proj = torch.as_tensor(synthetic.fcpe_state(13, 1, 512)["decoder._layers.0.attn.fast_attention.projection_matrix"],
                           device=dev)
    stages = {
        "fcpe": lambda: eng.fcpe(audio, 0.006),
        "rmvpe": lambda: eng.rmvpe(audio),
        "performer_attention": lambda: eng.performer_attention(q, k, v, proj),
    }
    res = {}
    for name, fn in stages.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        res[name] = round(a.elapsed_time(b) / args.reps, 4)
        print(f"{name:20s} {res[name]:8.4f} ms", flush=True)
    M = int(proj.shape[0])
    flops = 8.0 * F * M * 64 * 2 * 4  # dash and the second product, for the keys and for the queries
    hbm = 4.0 * (4 * 8 * F * 64 + 2 * 8 * M * 65)  # q, k, v read, out written, ctx / ksum written and read
    print(json.dumps({"frames": F, "reps": args.reps, "ms": res, "attention_gflop": round(flops / 1e9, 3),
                      "attention_hbm_mb": round(hbm / 1e6, 2)}))
    eng.close()


if __name__ == "__main__":
    main()
