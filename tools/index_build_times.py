"""Device time of the index build (csrc/kmeans.hip, index_build.cpp) at the reference's largest unreduced size, beside
a CPU baseline and the search route that was the only way to a nearest centroid before (diagnostic, not product code).

  assign_200k     one nearest-centroid pass, 200 000 x 768 against 5128 centroids (extract_index.py:43, :58:
                  the most rows that are not reduced first, and their n_ivf); HIP events around each pass after a
                  warm-up, the median of --reps passes; achieved TFLOP/s = 2 n nlist d / time, beside the 157.3 TF
                  fp32-matrix ceiling
  build_200k      the whole rvcx_index_build at that size: 10 Lloyd iterations + the final assignment and pack
                  (host clock around the call, which ends synchronised); median of --build-reps
  cpu_200k        the same single pass as torch matmul + argmin in fp32 on --cpu-threads threads of this machine,
                  in chunks of 8192 queries (the stand-in for faiss-cpu, which is not installed); median of --cpu-reps
  fused_20k /     20 000 x 768 against 1024 centroids: the fused kernel, and rvcx_index_search(k = 1) over an index
  search_20k      that stores exactly its own centroids, one per list (k_ivf_coarse writing the [n][nlist] matrix +
                  k_ivf_probe with nprobe 1 + a one-vector k_ivf_scan per query); the two alternate, median of --reps

    python tools/index_build_times.py [--out profiles/index_build_times.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "retrieval-based-voice-conversion-mlx_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TF = 157.3


def clock_state():
    """The device's clocks as the system tool reports them (read only), for the record beside the timings."""
    props = torch.cuda.get_device_properties(0)
    khz = getattr(props, "clock_rate", None)
    lines = [f"device: {torch.cuda.get_device_name(0)}, {props.multi_processor_count} CUs"
             + (f"; max engine clock {khz / 1000:.0f} MHz" if khz else "")]
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        lines += [ln.strip() for ln in out.splitlines() if "clk" in ln.lower()]
    except (OSError, subprocess.SubprocessError) as e:
        lines.append(f"rocm-smi --showclocks unavailable: {e}")
    return lines


def clustered(n, d, seed, dev, ncl=24):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centers = torch.randn((ncl, d), generator=g) * 2
    which = torch.randint(0, ncl, (n,), generator=g)
    return (centers[which] + torch.randn((n, d), generator=g)).to(dev)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build_times.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--build-reps", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--rows", type=int, default=200_000)
    args = ap.parse_args()
    from oracle import ivf
    from rvcx.engine import Engine
    from rvcx.infer.index import plan_index

    dev = torch.device("cuda:0")
    eng = Engine(0)
    lines = ["index build timings (tools/index_build_times.py)"] + clock_state()
    res = {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # ---- the largest unreduced case
    n, d = args.rows, 768
    reduce, nlist = plan_index(n)
    assert not reduce
    x = clustered(n, d, 1, dev)
    cent = x[torch.randperm(n, generator=torch.Generator().manual_seed(2))[:nlist].to(dev)].contiguous()
    flop = 2.0 * n * nlist * d
    ms = timed(lambda: eng.kmeans_assign(x, cent, want_dist=False), args.reps)
    med = float(np.median(ms))
    res["assign_200k"] = {"n": n, "d": d, "nlist": nlist, "median_ms": med, "min_ms": min(ms), "max_ms": max(ms),
                          "tflops": flop / med / 1e9}
    say(f"assign  {n} x {d} vs {nlist} centroids: median {med:.2f} ms (passes {min(ms):.2f} .. {max(ms):.2f}) = "
        f"{flop / med / 1e9:.1f} TFLOP/s of the {PEAK_TF} TF fp32-matrix ceiling ({flop / med / 1e9 / PEAK_TF:.1%})")

    def build():
        eng.index_build(x, nlist, niter=10, seed=0)

    build()
    torch.cuda.synchronize()
    bs = []
    for _ in range(args.build_reps):
        t0 = time.perf_counter()
        build()
        torch.cuda.synchronize()
        bs.append((time.perf_counter() - t0) * 1e3)
    res["build_200k"] = {"niter": 10, "median_ms": float(np.median(bs)), "min_ms": min(bs), "max_ms": max(bs)}
    say(f"build   {n} x {d} into {nlist} lists, 10 iterations + final add: median {np.median(bs):.1f} ms "
        f"(runs {min(bs):.1f} .. {max(bs):.1f}); 11 assignment passes alone are {11 * med:.1f} ms of it")
    gpu_ids = eng.host(eng.kmeans_assign(x, cent, want_dist=False)[0])
    eng.index_unload()

    # ---- the same pass on the CPU
    torch.set_num_threads(args.cpu_threads)
    xc, cc = x.cpu(), cent.cpu()
    cn = (cc * cc).sum(1)

    def cpu_pass():
        out = torch.empty(n, dtype=torch.int64)
        for i in range(0, n, 8192):
            s = cn[None, :] - 2.0 * (xc[i:i + 8192] @ cc.T)
            out[i:i + 8192] = s.argmin(1)
        return out

    cpu_pass()
    cs = []
    for _ in range(args.cpu_reps):
        t0 = time.perf_counter()
        cpu_ids = cpu_pass()
        cs.append((time.perf_counter() - t0) * 1e3)
    cmed = float(np.median(cs))
    agree = float((cpu_ids.numpy() == gpu_ids).mean())
    res["cpu_200k"] = {"threads": args.cpu_threads, "median_ms": cmed, "min_ms": min(cs), "max_ms": max(cs),
                       "tflops": flop / cmed / 1e9, "ids_equal_share": agree}
    say(f"cpu     the same pass, torch matmul + argmin fp32 on {args.cpu_threads} threads: median {cmed:.0f} ms "
        f"(passes {min(cs):.0f} .. {max(cs):.0f}) = {flop / cmed / 1e9:.2f} TFLOP/s; device pass is "
        f"{cmed / med:.0f}x faster; ids equal on {agree:.4%} of the rows")

    # ---- fused kernel vs the search route, 20 000 x 768 vs 1024 centroids
    n2, nl2 = 20_000, 1024
    x2 = x[:n2].contiguous()
    c2 = cent[:nl2].contiguous()
    c2h = c2.cpu().numpy()
    image = ivf.write_ivfflat(ivf.IvfFlat(d, nl2, 1, c2h, [c2h[l:l + 1] for l in range(nl2)],
                                          [np.array([l], np.int64) for l in range(nl2)]))
    eng.index_load(image)
    fused = lambda: eng.kmeans_assign(x2, c2, want_dist=False)  # noqa: E731
    search = lambda: eng.index_search(x2, 1)  # noqa: E731
    fused(), search()
    torch.cuda.synchronize()
    fm, sm = [], []
    for _ in range(args.reps):  # alternating
        fm += timed(fused, 1, warm=0)
        sm += timed(search, 1, warm=0)
    a_f = eng.host(fused()[0])
    a_s = eng.host(search()[1])[:, 0]
    same = float((a_f == a_s).mean())
    flop2 = 2.0 * n2 * nl2 * d
    fmed, smed = float(np.median(fm)), float(np.median(sm))
    res["fused_20k"] = {"median_ms": fmed, "min_ms": min(fm), "max_ms": max(fm), "tflops": flop2 / fmed / 1e9}
    res["search_20k"] = {"median_ms": smed, "min_ms": min(sm), "max_ms": max(sm), "ids_equal_share": same}
    say(f"fused   {n2} x {d} vs {nl2} centroids: median {fmed:.3f} ms (passes {min(fm):.3f} .. {max(fm):.3f}) = "
        f"{flop2 / fmed / 1e9:.1f} TFLOP/s")
    say(f"search  the same through rvcx_index_search(k=1) (k_ivf_coarse + k_ivf_probe + one-vector k_ivf_scan): median "
        f"{smed:.3f} ms (passes {min(sm):.3f} .. {max(sm):.3f}); fused is {smed / fmed:.1f}x faster; ids equal on "
        f"{same:.4%} of the rows")
    lines.append(json.dumps(res))
    print(json.dumps(res))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
