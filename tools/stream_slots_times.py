"""Device time of a realtime hop of a 16-slot group: the uniform hop through the old entry point, the same with index
retrieval on every stream, and hops with some slots idle beside plain groups of that many streams (diagnostic, not
product code).

The C5 geometry (read_chunk_size 96: 256 ms hops, 13920-sample convert buffers), seeded weights, f0_method "rmvpe",
drawn noise. HIP events around R back-to-back calls after a warm-up; all variants alternate within the run, `rounds`
times, and the mean per call of every round is kept: the figures printed are the mean over the rounds and their lowest
and highest value (the spread).

  uniform16            rvcx_rt_process (one rvcx_rt_opts) on 16 streams, index_rate 0
  index16              the same with index_rate 0.5 on all 16 streams (a 3000 x 768 IVF48 index, nprobe 1)
  index16_tiny         the same launches with index_rate 1e-9: the search and blend run, the features the synthesizer
                       sees stay what they are without retrieval (tells the cost of the retrieval launches apart from
                       what the retrieved values do to the rest of the hop)
  base_uniform16 /     the same two through another build of the library (--baseline-lib, e.g. the parent commit's
  base_index16         librvcx.so), in the same process and alternating with the rows above
  mixed16              rvcx_rt_process_v with 16 different option sets (keys, protect, autotune, volume envelope and
                       index rates 0 .. 1 mixed; no proposed pitch, so no host sync)
  active16/8/4_of16    rvcx_rt_process_v on the 16-slot group with 16, 8 (every 2nd) and 4 (every 4th) slots active
  plain8 / plain4      rvcx_rt_process on groups created with 8 and 4 streams

    python tools/stream_slots_times.py [--reps 20] [--rounds 5] [--baseline-lib PATH]
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
    ap.add_argument("--baseline-lib", default=None, help="a librvcx.so of another build to time beside this one")
    args = ap.parse_args()
    from oracle import ivf
    from rvcx import _lib, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup, hop_arguments
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    centers = rng.standard_normal((24, 768)).astype(np.float32) * 2
    vecs = (centers[rng.integers(0, 24, 3000)] + rng.standard_normal((3000, 768)).astype(np.float32))
    image = ivf.write_ivfflat(ivf.build_ivfflat(vecs.astype(np.float32), nlist=48, nprobe=1))

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
        e.index_load(image)
        return e

    geom = dict(read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5, silent_threshold=-90.0)
    eng = engine()
    base = engine(args.baseline_lib) if args.baseline_lib else None
    g16, g8, g4 = (StreamGroup(eng, n, **geom) for n in (16, 8, 4))
    gidx, gtiny, gmix = (StreamGroup(eng, B, **geom) for _ in range(3))
    blk = g16.geometry["block48"]
    hops = 4  # distinct input blocks, cycled
    x48 = torch.as_tensor(np.stack([synthetic.speech_like(blk * hops, seed=300 + s, sr=48000) for s in range(B)]),
                          dtype=torch.float32).to(dev)
    count = {"hop": 0}

    def block(n):
        h = count["hop"] % hops
        count["hop"] += 1
        return x48[:n, h * blk:(h + 1) * blk].contiguous()

    def old_entry(e, g, o):  # rvcx_rt_process, as a caller of either build reaches it
        def run():
            x = block(g.n_streams)
            e._check(e.lib.rvcx_rt_process(e.ctx, g.handle, x.data_ptr(), g.sids, ctypes.byref(o), None, None,
                                           ctypes.c_uint64(count["hop"]), g.out.data_ptr(), g.vol.data_ptr(),
                                           g.offs.data_ptr(), e.stream()), "rt_process")
        return run

    def per_slot(g, opts, active=None):  # rvcx_rt_process_v
        arr, act = hop_arguments(g.n_streams, opts, active)

        def run():
            x = block(g.n_streams)
            eng._check(eng.lib.rvcx_rt_process_v(eng.ctx, g.handle, x.data_ptr(), g.sids, arr, act, None, None,
                                                 ctypes.c_uint64(count["hop"]), g.out.data_ptr(), g.vol.data_ptr(),
                                                 g.offs.data_ptr(), eng.stream()), "rt_process_v")
        return run

    plain, idx = g16.opts(index_rate=0.0), g16.opts(index_rate=0.5)
    mixed = [g16.opts(f0_up_key=(s % 7) - 3, protect=0.5 if s % 2 else 0.33, index_rate=(s % 5) / 4,
                      volume_envelope=1.0 if s % 3 else 0.5, f0_autotune=s % 4 == 3, f0_autotune_strength=0.7)
             for s in range(B)]
    stages = {"uniform16": old_entry(eng, g16, plain), "index16": old_entry(eng, gidx, idx),
              "index16_tiny": old_entry(eng, gtiny, g16.opts(index_rate=1e-9))}
    if base is not None:
        b16, bidx = StreamGroup(base, B, **geom), StreamGroup(base, B, **geom)
        stages["base_uniform16"] = old_entry(base, b16, plain)
        stages["base_index16"] = old_entry(base, bidx, idx)
    stages["mixed16"] = per_slot(gmix, mixed)
    stages["active16_of16"] = per_slot(g16, plain, [True] * B)
    stages["active8_of16"] = per_slot(g16, plain, [s % 2 == 0 for s in range(B)])
    stages["active4_of16"] = per_slot(g16, plain, [s % 4 == 0 for s in range(B)])
    stages["plain8"] = old_entry(eng, g8, plain)
    stages["plain4"] = old_entry(eng, g4, plain)
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
        print(f"{name:15s} mean {res[name]['mean_ms']:8.4f} ms  (rounds {min(v):.4f} .. {max(v):.4f})", flush=True)
    print(json.dumps({"slots": B, "reps": args.reps, "rounds": args.rounds, "baseline": bool(base), "ms": res}))
    for g in (g16, g8, g4, gidx, gtiny, gmix):
        g.close()
    eng.close()
    if base is not None:
        b16.close()
        bidx.close()
        base.close()


if __name__ == "__main__":
    main()
