"""The three elementwise kernels of the RefineGAN decoder (csrc/refinegan.hip) stated in plain torch at float64, with the
a-priori fp32 rounding bound of each (test helper, no GPU needed). tests/test_gpu_refinegan_kernels.py holds the device
to the bounds; tests/test_refinegan_cpu.py shows that the bounds refuse the mistakes such kernels make.

    resample_dw   y[b][t][c] = sum_k x[b][t orig + k - width][c] ker[k], zero outside the input: an fp32 fma chain of K
                  terms, so |err| <= (K + 2) 2^-24 sum_k |x ker| per output
    lerp_up_cat   cat(interpolate(leaky_relu(x, slope), scale_factor = rate, "linear"), skip): the source index takes two
                  roundings, the blend three: |err| <= (2 ulp32(src + 1) + 4 2^-24) (|a| + |b|), a and b the two
                  activated neighbours; the skip columns are copies
    adain         v = leaky_relu(x + eps[b][c][t] w[c], slope); store / add / (y + v) / div:
                  |err| <= 4 2^-24 (|x| + |eps w| + |y0|)

Arrays are time-major as the decoder holds them (x [B][T][C]); the noise is in the reference's layout [B][C][T].
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # fp32 unit roundoff
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]

RATES = (2, 8, 10, 12)  # every upsample rate of the 48 / 40 / 32 kHz lists
UNIT_TAPS = ((2, 3), (3, 5), (12, 40))  # (orig, width) of the random-tap cases


# ----------------------------------------------------------------- the decoder's configurations and seeded inputs
LENGTHS, SEED, SEED_W = (24, 17, 1), 7, 7  # the point of tests/test_gpu_synth_configs.py, synth_configs.SEED_W
_BASE = {"rg_48k": None, "rg_40k": "v2_40k", "rg_32k": "v2_32k"}
_W = {}


def config(name, vocoder="RefineGAN"):
    """rg_48k / rg_40k / rg_32k: the 48 / 40 / 32 kHz v2 lists with `vocoder`."""
    import dataclasses

    from rvcx.config import SYNTH_48K_V2
    from synth_configs import CONFIGS

    base = SYNTH_48K_V2 if _BASE[name] is None else CONFIGS[_BASE[name]]
    return dataclasses.replace(base, vocoder=vocoder)


def weights_for(name, vocoder="RefineGAN"):
    """normalize_state(synthetic.synth_state(SEED_W, cfg)), built once per (configuration, decoder), never modified."""
    if (name, vocoder) not in _W:
        from rvcx import synthetic
        from rvcx.weights import normalize_state

        _W[(name, vocoder)] = normalize_state(synthetic.synth_state(SEED_W, config(name, vocoder)))
    return _W[(name, vocoder)]


def noise(cfg, B, T, rng):
    """The decoder's flat source noise for B rows of T frames, drawn in oracle.synth.refinegan_noise_sizes order: the
    source's randn, U(0, 1) for the initial phase, randn per AdaIN [B][C][T_stage]."""
    from oracle.synth import refinegan_noise_sizes

    s = refinegan_noise_sizes(cfg, B, T)
    return np.concatenate([rng.standard_normal(s[0]), rng.random(s[1])] +
                          [rng.standard_normal(n) for n in s[2:]]).astype(np.float32)


def synth_case(cfg, lengths=LENGTHS, seed=SEED):
    """parity_anchor.synth_case(cfg=) with eps_src in the RefineGAN layout (PCG64(seed + 1))."""
    import parity_anchor as pa

    c = pa.synth_case(lengths, seed, cfg=cfg)
    c["eps_src"] = noise(cfg, len(lengths), int(lengths[0]), np.random.Generator(np.random.PCG64(seed + 1)))
    return c


def row_noise(cfg, eps_src, B, T, b, Tb=None):
    """Row b's own noise (a B = 1 call of Tb <= T frames) cut out of a batch's flat blocks: the source randn
    [B][T upp] and every AdaIN block [B][C][T_stage] keep their first Tb frames' samples, the phase its entry."""
    from oracle.synth import refinegan_noise_sizes

    Tb = T if Tb is None else Tb
    sizes = refinegan_noise_sizes(cfg, B, T)
    parts = np.split(np.asarray(eps_src, np.float32).reshape(-1), np.cumsum(sizes)[:-1])
    out = [parts[0].reshape(B, T * cfg.upp)[b, :Tb * cfg.upp], parts[1].reshape(B)[b:b + 1]]
    ch, t = 512, T
    k = 2
    for r in cfg.upsample_rates:
        ch, t = ch // 2, t * r
        for _ in range(6):
            out.append(parts[k].reshape(B, ch, t)[b, :, :t // T * Tb].reshape(-1))
            k += 1
    return np.concatenate(out)


def real_taps(r):
    """(float32 taps [2 width + r], width) of RefineGAN's resample(r -> 1) (refinegan.py:410-419), from the oracle."""
    from oracle.realtime import sinc_resample_kernel

    k, width, orig, new = sinc_resample_kernel(r, 1, 64, 0.9475937167399596, torch.float32, "sinc_interp_kaiser",
                                               14.769656459379492)
    assert (orig, new) == (r, 1) and k.shape == (1, 1, 2 * width + r)
    return k.reshape(-1).numpy().copy(), width


def resample_lengths(orig, width):
    K = 2 * width + orig
    return sorted({1, max(orig - 1, 1), max(width, 1), K, 3 * K + 5})


def resample_ref(x, ker, orig, width):
    """x [B][T][C], ker [K] float32 -> (y [B][ceil(T / orig)][C] float64, bound): F.conv1d of the padded rows."""
    xt = torch.from_numpy(np.asarray(x, np.float32)).double().permute(0, 2, 1)
    B, C, T = xt.shape
    k = torch.from_numpy(np.asarray(ker, np.float32)).double()
    assert k.numel() == 2 * width + orig
    xp = F.pad(xt, (width, width + orig)).reshape(B * C, 1, -1)
    T_out = -(-T // orig)
    y = F.conv1d(xp, k[None, None], stride=orig)[..., :T_out]
    mag = F.conv1d(xp.abs(), k.abs()[None, None], stride=orig)[..., :T_out]
    tm = lambda a: a.reshape(B, C, T_out).permute(0, 2, 1).contiguous().numpy()  # noqa: E731
    return tm(y), (k.numel() + 2) * U * tm(mag)


def lerp_ref(x, skip, rate, slope=0.2, align_corners=False):
    """x [B][T][C] (the C columns read), skip [B][T rate][Cd] float32 -> (y [B][T rate][C + Cd] float64, bound over
    the C interpolated columns)."""
    a = F.leaky_relu(torch.from_numpy(np.asarray(x, np.float32)).double(), slope)
    T = a.shape[1]
    if align_corners:
        up = F.interpolate(a.permute(0, 2, 1), size=T * rate, mode="linear", align_corners=True)
    else:
        up = F.interpolate(a.permute(0, 2, 1), scale_factor=float(rate), mode="linear")
    up = up.permute(0, 2, 1)
    y = torch.cat([up, torch.from_numpy(np.asarray(skip, np.float32)).double()], dim=2).numpy()
    src = np.maximum((np.arange(T * rate) + 0.5) / rate - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, T - 1)
    aa = np.abs(a.numpy())
    ulp = np.spacing((src + 1.0).astype(np.float32)).astype(np.float64)
    bound = (2.0 * ulp + 4.0 * U)[None, :, None] * (aa[:, i0] + aa[:, i1])
    return y, bound


def adain_ref(x, w, eps, y0, mode, div=3.0, slope=0.2):
    """x, y0 [B][T][C], w [C], eps [B][C][T] float32 -> (y float64, bound); mode 0 store, 1 add, 2 (y0 + v) / div."""
    d = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double()  # noqa: E731
    x, w, eps, y0 = d(x), d(w), d(eps), d(y0)
    nz = eps.permute(0, 2, 1) * w
    v = F.leaky_relu(x + nz, slope)
    y = v if mode == 0 else (y0 + v if mode == 1 else (y0 + v) / div)
    bound = 4.0 * U * (x.abs() + nz.abs() + (y0.abs() if mode else 0.0))
    return y.numpy(), bound.numpy()


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact zero is within any bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-300))))


def shares_run(a, b, n=8):
    """True when some n consecutive values of a appear, in order, anywhere in b (bit patterns)."""
    win = lambda v: np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(  # noqa: E731
        np.asarray(v, np.float32).reshape(-1).view(np.uint32), n)).view(np.dtype((np.void, 4 * n))).reshape(-1)
    return bool(np.intersect1d(win(a), win(b)).size)
