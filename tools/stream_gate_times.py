"""Device time of a realtime hop of a 16-stream group with and without the noise gate (rvcx_rt_set_clean), and
of the gate alone (diagnostic, not product code).

The C5 geometry (read_chunk_size 96: 256 ms hops, 87 frames, 41760-sample model rows), seeded weights, f0_method
"rmvpe", drawn noise, index_rate 0. HIP events around R back-to-back calls after a warm-up; all variants alternate
within the run, `rounds` times, and the mean per call of every round is kept: the figures printed are the mean over the
rounds and their lowest and highest value (the spread).

  uniform16          rvcx_rt_process (one rvcx_rt_opts) on 16 streams, no stream cleaning
  base_uniform16 /   the same through another build of the library (--baseline-lib, e.g. the parent commit's
  base_uniform16_b   librvcx.so) on two groups of its own, alternating with the rows above: the second tells that
                     build's own run-to-run spread
  nowindow16         uniform16 with the generator's output window off (rvcx_set_dec_window 0): what a cleaning hop
                     loses before the gate does anything
  clean16            all 16 streams cleaning at strength 0.5 (rvcx_rt_set_clean(-1, 1, 0.5) once, before the hops)
  gate_alone         rvcx_spectral_gate on [16][41760] at 48 kHz, strength 0.5: four launches (forward, statistics,
                     back, overlap-add) whatever the number of rows

    python tools/stream_gate_times.py [--reps 20] [--rounds 5] [--baseline-lib PATH]
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
GATE_LAUNCHES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="a librvcx.so of another build to time beside this one")
    args = ap.parse_args()
    from rvcx import _lib, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")

    def engine(lib_path=None):
        if lib_path is None:
            e = Engine(0)
        else:  # an Engine bound to the other build: Engine() takes whatever _lib.load() returns
            keep, _lib._lib = _lib._lib, _lib.load(lib_path)
            try:
                e = Engine(0)
            finally:
                _lib._lib = keep
        e.load_synth(normalize_state(synthetic.synth_state(2)), SYNTH_48K_V2)
        e.load_hubert(normalize_state(synthetic.hubert_state(4)))
        e.load_rmvpe(normalize_state(synthetic.rmvpe_state(5)))
        return e

    geom = dict(read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5, silent_threshold=-90.0)
    eng = engine()
    base = engine(args.baseline_lib) if args.baseline_lib else None
    g_plain, g_now, g_clean = (StreamGroup(eng, B, **geom) for _ in range(3))
    blk = g_plain.geometry["block48"]
    n_model = g_plain.geometry["frames"] * eng.upp
    hops = 4  # distinct input blocks, cycled
    x48 = torch.as_tensor(np.stack([synthetic.speech_like(blk * hops, seed=300 + s, sr=48000) for s in range(B)]),
                          dtype=torch.float32).to(dev)
    count = {"hop": 0}

    def hop(e, g, o, window=True):  # rvcx_rt_process, as a caller of either build reaches it
        def run():
            h = count["hop"] % hops
            count["hop"] += 1
            x = x48[:, h * blk:(h + 1) * blk].contiguous()
            if not window:
                e.set_dec_window(False)
            e._check(e.lib.rvcx_rt_process(e.ctx, g.handle, x.data_ptr(), g.sids, ctypes.byref(o), None, None,
                                           ctypes.c_uint64(count["hop"]), g.out.data_ptr(), g.vol.data_ptr(),
                                           g.offs.data_ptr(), e.stream()), "rt_process")
            if not window:
                e.set_dec_window(True)
        return run

    rows = torch.as_tensor(np.stack([synthetic.speech_like(n_model, seed=400 + s, sr=48000) for s in range(B)]),
                           dtype=torch.float32).to(dev)
    gated = torch.empty_like(rows)
    strength = (ctypes.c_float * B)(*([0.5] * B))

    def gate_alone():
        eng._check(eng.lib.rvcx_spectral_gate(eng.ctx, rows.data_ptr(), B, n_model, n_model, 48000, strength,
                                              gated.data_ptr(), n_model, None, eng.stream()), "spectral_gate")

    plain = g_plain.opts(index_rate=0.0)
    stages = {"uniform16": hop(eng, g_plain, plain)}
    if base is not None:
        b1, b2 = StreamGroup(base, B, **geom), StreamGroup(base, B, **geom)
        stages["base_uniform16"] = hop(base, b1, plain)
        stages["base_uniform16_b"] = hop(base, b2, plain)
    stages["nowindow16"] = hop(eng, g_now, plain, window=False)
    eng._check(eng.lib.rvcx_rt_set_clean(eng.ctx, g_clean.handle, -1, 1, 0.5), "rt_set_clean")
    stages["clean16"] = hop(eng, g_clean, plain)
    stages["gate_alone"] = gate_alone
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
        print(f"{name:17s} mean {res[name]['mean_ms']:8.4f} ms  (rounds {min(v):.4f} .. {max(v):.4f})", flush=True)
    print(json.dumps({"streams": B, "reps": args.reps, "rounds": args.rounds, "baseline": bool(base),
                      "gate_launches": GATE_LAUNCHES, "gate_rows": [B, n_model], "ms": res}))
    for g in (g_plain, g_now, g_clean):
        g.close()
    eng.close()
    if base is not None:
        b1.close()
        b2.close()
        base.close()


if __name__ == "__main__":
    main()
