"""Loading a folder of recordings: the host loader (scipy.signal.resample_poly, one file at a time) against the device
resampler (rvcx_resample_poly_v), and `infer_batch` end to end each way (diagnostic, not product code).

The job: the 64 lengths of tools/ragged_batch_times.py (2-30 s), written once to a temporary folder as 44.1 kHz stereo
int16 WAVs and once as 48 kHz mono int16. Every route is timed over the whole job with a host clock around work that
ends in a device synchronise, after one untimed warm-up pass; --reps passes, median and min .. max reported:
  (a) loop of host `load_audio` (the route before the device resampler; its own min .. max is the yardstick), each
      result uploaded as the pipeline would.
  (b) `load_audio(path, engine=)` per file.
  (c) `load_audio_device(paths, engine)`: what `infer_batch(device_load=True)` does, one launch per group.
  (d) `infer_batch` end to end, host-loaded and device-loaded, at batch 8 / max_pad 0.125 with ragged_f0=True
      (output files included: both routes write the same ones).
For (b) and (c) the parts are timed on their own as well: the file reads, the host-to-device copies and the kernel
alone (device events around the call on inputs already in HBM).
A route is called faster (slower) only if its median lies below (above) the other's min .. max.

    python tools/device_load_times.py [--reps 5] [--files 64] [--no-e2e] > profiles/device_load_times.txt
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

FORMATS = (("44.1 kHz stereo int16", 44100, 2), ("48 kHz mono int16", 48000, 1))


def write_job(folder, rate, ch, lengths):
    """One WAV per length (samples at 16 kHz): stretches of one speech-like signal, a channel c starting c seconds in."""
    from scipy.io import wavfile

    from rvcx import synthetic

    longest = max(lengths) * rate // 16000
    base = np.round(synthetic.speech_like(longest + ch * rate, seed=3000, sr=rate) * 32767.0).astype(np.int16)
    paths = []
    for i, n16 in enumerate(lengths):
        n = n16 * rate // 16000
        x = np.stack([base[c * rate: c * rate + n] for c in range(ch)], axis=1)
        paths.append(os.path.join(folder, f"utt{i:02d}.wav"))
        wavfile.write(paths[-1], rate, x[:, 0] if ch == 1 else x)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    from ragged_batch_times import job_lengths
    from scipy.io import wavfile

    from rvcx import _lib, resample, synthetic
    from rvcx.config import SYNTH_48K_V2
    from rvcx.infer import RVCX
    from rvcx.infer.infer import load_audio, load_audio_device
    from rvcx.weights import normalize_state

    dev = torch.device("cuda:0")
    rvc = RVCX(synth_state=normalize_state(synthetic.synth_state(2)), synth_cfg=SYNTH_48K_V2,
               hubert_state=normalize_state(synthetic.hubert_state(4)),
               rmvpe_state=normalize_state(synthetic.rmvpe_state(5)))
    eng = rvc.engine
    ns = job_lengths()[: args.files]
    seconds = sum(ns) / 16000
    print(f"library: {os.path.relpath(_lib.LIB_PATH, ROOT)}")
    print(f"job: {len(ns)} files, {min(ns) / 16000:.2f} .. {max(ns) / 16000:.2f} s, {seconds:.1f} s of audio; "
          f"{args.reps} timed passes after one warm-up; host threads: {torch.get_num_threads()}")
    res = {}

    def once(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def timed(*fns):
        for fn in fns:
            fn()
        out = [[] for _ in fns]
        for _ in range(args.reps):
            for k, fn in enumerate(fns):
                out[k].append(once(fn))
        return out

    def report(name, t, ref=None):
        med = statistics.median(t)
        verdict = ""
        if ref is not None:
            verdict = "faster" if med < min(ref) else ("slower" if med > max(ref) else "inside the other's min .. max")
        res[name] = [round(x, 5) for x in t]
        print(f"  {name:58s} median {med * 1e3:9.2f} ms  min {min(t) * 1e3:9.2f}  max {max(t) * 1e3:9.2f}  {verdict}",
              flush=True)

    def kernel_ms(x, dtype, ch, n_rows, ldx, up, down):
        """The resampling call alone on inputs in HBM (device events; the first call warms up)."""
        h = torch.as_tensor(np.array(resample.taps(up, down)), device=dev)
        B = len(n_rows)
        ldy = max(resample.plan(n, up, down)[2] for n in n_rows)
        y = torch.empty((B, ldy), dtype=torch.float64, device=dev)
        no = (ctypes.c_int64 * B)()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps + 1):
            a.record()
            eng._check(eng.lib.rvcx_resample_poly_v(eng.ctx, x.data_ptr(), dtype, ch, (ctypes.c_int64 * B)(*n_rows),
                                                    ldx, B, up, down, h.data_ptr(), h.numel(), y.data_ptr(), ldy, no,
                                                    eng.stream()), "resample_poly")
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms[1:]

    with tempfile.TemporaryDirectory() as tmp:
        for label, rate, ch in FORMATS:
            src = os.path.join(tmp, f"in_{rate}")
            os.makedirs(src)
            paths = write_job(src, rate, ch, ns)
            up, down = resample.reduce(16000, rate)
            print(f"{label} ({up}/{down}), {sum(os.path.getsize(p) for p in paths) / 2 ** 20:.1f} MiB of files")
            data = [wavfile.read(p)[1] for p in paths]

            def host_loop():
                for p in paths:
                    eng._dev(load_audio(p), torch.float64)

            def device_loop():
                for p in paths:
                    load_audio(p, engine=eng)

            def device_grouped():
                load_audio_device(paths, eng)

            def reads():
                for p in paths:
                    wavfile.read(p)

            def copies():
                for d in data:
                    torch.as_tensor(d, device=dev)

            frames = [len(d) for d in data]
            image = np.zeros((len(data), max(frames) * ch), dtype=np.int16)

            def copy_grouped():
                for r, d in enumerate(data):
                    image[r, : d.size] = d.reshape(-1)
                torch.as_tensor(image, device=dev)

            t_a, t_b, t_c, t_r, t_h, t_g = timed(host_loop, device_loop, device_grouped, reads, copies, copy_grouped)
            report("(a) loop of host load_audio + upload", t_a)
            report("(b) loop of load_audio(engine=)", t_b, t_a)
            report("(c) load_audio_device, one launch per group", t_c, t_a)
            report("    file reads alone (b, c)", t_r)
            report("    host-to-device copies alone, per file (b)", t_h)
            report("    padded image + one copy alone (c)", t_g)
            each = [kernel_ms(torch.as_tensor(d, device=dev), 2, ch, [f], f, up, down) for d, f in zip(data, frames)]
            report("    kernel alone, per file, summed (b)", [sum(k[r] for k in each) / 1e3 for r in range(args.reps)])
            grouped = kernel_ms(torch.as_tensor(image, device=dev), 2, ch, frames, max(frames), up, down)
            report("    kernel alone, one launch (c)", [g / 1e3 for g in grouped])
            if not args.no_e2e:
                kw = dict(batch=8, max_pad=0.125, ragged_f0=True, pitch=2.0, protect=0.33)
                out_h, out_d = os.path.join(tmp, f"out_h_{rate}"), os.path.join(tmp, f"out_d_{rate}")
                t_eh, t_ed = timed(lambda: rvc.infer_batch(src, out_h, **kw),
                                   lambda: rvc.infer_batch(src, out_d, device_load=True, **kw))
                report("(d) infer_batch, host loader", t_eh)
                report("(d) infer_batch(device_load=True)", t_ed, t_eh)
    print(json.dumps(res))
    rvc.close()


if __name__ == "__main__":
    main()
