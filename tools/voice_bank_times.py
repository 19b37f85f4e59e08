"""What serving several voices from one context costs (diagnostic, not product code): device time of a realtime hop of
a 16-slot group with 1 .. 16 voices in use, the same against separate engines, the host time of a voice switch and the
memory a voice holds.

The C5 geometry (read_chunk_size 96: 256 ms hops, 13920-sample convert buffers), seeded weights, f0_method "rmvpe",
drawn noise, index_rate 0. HIP events around `reps` back-to-back calls after a warm-up; all variants alternate within
the run, `rounds` times, and the time per call of every round is kept: the figures printed are the median over the
rounds and their lowest and highest value.

  (a) uniform16          rvcx_rt_process on 16 streams of one voice
      base_uniform16     the same through another build of the library (--baseline-lib, e.g. the parent commit's
                         librvcx.so), in the same process and alternating with the row above
  (b) voices2/4/8/16     the 16-slot group with that many voices in use, slot b on voice b mod K (interleaved: the row
                         map is passed), through rvcx_rt_process_v
      voices4_blocks     4 voices in blocks of 4 slots (slot order: no row map)
  (c) engines4x4         what the bank replaces: 4 engines, each with its own HuBERT and RMVPE and one voice, 4 slots
                         each, run hop after hop; against voices4_blocks. HBM held by either (the device's free memory
                         before and after each was built and had run), in MiB
  (d) voice_select       host time of rvcx_voice_select between two resident voices, ns per call
  (e) weight_bytes / split_bytes of one 48 kHz v2 voice after a hop has used it

    python tools/voice_bank_times.py [--reps 10] [--rounds 5] [--baseline-lib PATH] > profiles/voice_bank_times.txt
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="a librvcx.so of another build to time beside this one")
    args = ap.parse_args()
    from rvcx import _lib, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.engine import Engine
    from rvcx.realtime import StreamGroup, hop_arguments
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    states = [normalize_state(synthetic.synth_state(s)) for s in (2, 3, 21, 22)]  # cycled: the values do not matter
    hubert, rmvpe = normalize_state(synthetic.hubert_state(4)), normalize_state(synthetic.rmvpe_state(5))

    def free_mib():
        torch.cuda.synchronize(dev)
        return torch.cuda.mem_get_info(dev)[0] / 2 ** 20

    def engine(n_voices=1, lib_path=None):
        if lib_path is None:
            e = Engine(0)
        else:  # an Engine bound to the other build: Engine() takes whatever _lib.load() returns
            keep, _lib._lib = _lib._lib, _lib.load(lib_path)
            try:
                e = Engine(0)
            finally:
                _lib._lib = keep
        e.load_synth(states[0], SYNTH_48K_V2)
        e.load_hubert(hubert)
        e.load_rmvpe(rmvpe)
        for k in range(1, n_voices):
            e.add_voice(states[k % len(states)], SYNTH_48K_V2)
        return e

    geom = dict(read_chunk_size=96, cross_fade_overlap_size=0.1, extra_convert_size=0.5, silent_threshold=-90.0)
    hops = 4  # distinct input blocks, cycled
    count = {"hop": 0}
    blk = 96 * 128
    x48 = torch.as_tensor(np.stack([synthetic.speech_like(blk * hops, seed=300 + s, sr=48000) for s in range(B)]),
                          dtype=torch.float32).to(dev)

    def block(n, first=0):
        h = count["hop"] % hops
        count["hop"] += 1
        return x48[first:first + n, h * blk:(h + 1) * blk].contiguous()

    def old_entry(e, g, o, first=0):  # rvcx_rt_process, as a caller of either build reaches it
        def run():
            x = block(g.n_streams, first)
            e._check(e.lib.rvcx_rt_process(e.ctx, g.handle, x.data_ptr(), g.sids, ctypes.byref(o), None, None,
                                           ctypes.c_uint64(count["hop"]), g.out.data_ptr(), g.vol.data_ptr(),
                                           g.offs.data_ptr(), e.stream()), "rt_process")
        return run

    def per_slot(e, g, o):  # rvcx_rt_process_v
        arr, act = hop_arguments(g.n_streams, o, None)

        def run():
            x = block(g.n_streams)
            e._check(e.lib.rvcx_rt_process_v(e.ctx, g.handle, x.data_ptr(), g.sids, arr, act, None, None,
                                             ctypes.c_uint64(count["hop"]), g.out.data_ptr(), g.vol.data_ptr(),
                                             g.offs.data_ptr(), e.stream()), "rt_process_v")
        return run

    def warm(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)

    stages, groups, engines = {}, [], []
    held = {}
    # (c) first, so that each side's memory is read on a device that holds nothing else of this process
    f0 = free_mib()
    one = engine(4)
    g = StreamGroup(one, B, voices=[b // 4 for b in range(B)], **geom)
    plain = g.opts(index_rate=0.0)
    stages["voices4_blocks"] = per_slot(one, g, plain)
    warm(stages["voices4_blocks"])
    held["one engine, 16 slots, 4 voices"] = f0 - free_mib()
    groups.append(g), engines.append(one)
    f0 = free_mib()
    four = [engine(1) for _ in range(4)]
    g4 = [StreamGroup(e, 4, **geom) for e in four]
    runs4 = [old_entry(e, gg, plain, first=4 * k) for k, (e, gg) in enumerate(zip(four, g4))]

    def engines4x4():
        for r in runs4:
            r()
    stages["engines4x4"] = engines4x4
    warm(engines4x4)
    held["four engines, 4 slots each"] = f0 - free_mib()
    groups += g4
    engines += four
    # (a), (b)
    eng = engine(B)
    engines.append(eng)
    g16 = StreamGroup(eng, B, **geom)
    groups.append(g16)
    stages["uniform16"] = old_entry(eng, g16, plain)
    if args.baseline_lib:
        base = engine(1, args.baseline_lib)
        gb = StreamGroup(base, B, **geom)
        engines.append(base), groups.append(gb)
        stages["base_uniform16"] = old_entry(base, gb, plain)
    for K in (2, 4, 8, 16):
        gk = StreamGroup(eng, B, voices=[b % K for b in range(B)], **geom)
        groups.append(gk)
        stages[f"voices{K}"] = per_slot(eng, gk, plain)
    for name, fn in stages.items():
        warm(fn)
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
    for e in engines:
        e.check_device_status()
    res = {}
    for name in sorted(per_round, key=lambda k: ("base" in k, k)):
        v = per_round[name]
        res[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        print(f"{name:16s} median {res[name]['median_ms']:8.4f} ms  (rounds {min(v):.4f} .. {max(v):.4f})", flush=True)
    for k, v in held.items():
        print(f"HBM held, {k}: {v:.0f} MiB", flush=True)
    # (d) the host time of a voice switch
    n = 20000
    t0 = time.perf_counter()
    for i in range(n):
        eng.lib.rvcx_voice_select(eng.ctx, 1 + (i & 1))
    select_ns = (time.perf_counter() - t0) / n * 1e9
    eng.select_voice(0)
    print(f"voice_select: {select_ns:.0f} ns per call (ctypes call included)", flush=True)
    # (e)
    info = eng.voice_info(1)
    print(f"one 48 kHz v2 voice: weight_bytes {info['weight_bytes']} ({info['weight_bytes'] / 2 ** 20:.1f} MiB), "
          f"split_bytes {info['split_bytes']} ({info['split_bytes'] / 2 ** 20:.1f} MiB)", flush=True)
    print(json.dumps({"slots": B, "reps": args.reps, "rounds": args.rounds, "baseline": bool(args.baseline_lib),
                      "ms": res, "hbm_mib": {k: round(v) for k, v in held.items()},
                      "voice_select_ns": round(select_ns), "weight_bytes": info["weight_bytes"],
                      "split_bytes": info["split_bytes"]}))
    for g in groups:
        g.close()
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
