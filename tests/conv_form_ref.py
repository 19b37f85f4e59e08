"""The 1-D contraction forms the runtime issues, stated in torch at any dtype (test helper, no GPU needed).

`ref(d, dtype)` evaluates one form on logical arrays (no strides: x [B][G][T_in][C_in], w [G][taps][N][C_in], ...) with
the semantics documented at ConvArgs (csrc/conv_kernels.h) and spelled out by epilogue_store (csrc/conv_common.h):

    input   pre(x) * pre_mask, zero outside [0, T_in); row of output m, tap k: m stride - pad + k dil
    value   acc = sum x W; v = acc + bias; RES_ADD_PRE: v += R; v *= alpha; v = act(v);
            RES_ADD_POST: v += R; RES_RSUB_POST: v = R - v; ACC_ADD: y0 + v; ACC_ADD_DIV: (y0 + v) / acc_div;
            noise: v += nz_w[c] har[(m nz_u + p) nz_stride] + nz_b[c] at column p nz_C + c; v *= mask (last)
    gate    y[c] = tanh(v[c] + g[c]) sigmoid(v[c + H] + g[c + H]), v = acc + bias
    LN      y = LN(res + act(alpha (acc + bias)) mask) ln_g + ln_b over the N columns (biased variance)

CASES is the table tests/test_gpu_conv_forms.py runs on the device and tests/test_conv_form_ref_cpu.py proves
sensitive: one row per runtime call site, at the smallest shape that still reaches the site's kernel paths, and the
edge forms of the LDS-staged families' gather that no site reaches (the lds.* rows). `make`
draws a case's inputs, `place` / `gather` move logical arrays into and out of strided buffers whose every other
element is a guard, `mutate` applies one of the deviations a wrong kernel could carry.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

NONE, LRELU, RELU, GELU, TANH, SIGMOID, LOGCLAMP = range(7)  # Act (csrc/kernel_base.h)
RES_NONE, RES_ADD_PRE, RES_ADD_POST, RES_RSUB_POST = range(4)
ACC_STORE, ACC_ADD, ACC_ADD_DIV = range(3)
SENTINEL = np.array([0xDEADBEEF], np.uint32).view(np.float32)[0]  # finite, never a result
ALPHA192 = float(np.float32(np.sqrt(192.0)))

ALL5 = ("policy", "f32", "emu", "wsb", "gs")
ALL6 = ALL5 + ("wst",)


def _c(name, site, routes, **kw):
    d = dict(name=name, site=site, routes=routes, B=1, G=1, taps=1, dil=1, pad=0, stride=1, bias=True, alpha=1.0,
             act=NONE, slope=0.0, pre_act=NONE, pre_slope=0.0, res=None, res_bcast=False, res_inplace=False,
             acc=ACC_STORE, acc_div=1.0, gate=False, ln=False, nz=None, pre_mask=False, mask=False, lengths=None,
             flat=None, wspread=False, nonneg=False, x_col0=0, y_col0=0, ln_eps=1e-5)
    d.update(kw)
    nat = (d["T_in"] + 2 * d["pad"] - d["dil"] * (d["taps"] - 1) - 1) // d["stride"] + 1
    d.setdefault("T_out", nat)
    assert d["T_out"] <= nat
    d.setdefault("ldx", d["C_in"] * d["G"])
    d.setdefault("ldy", (d["N"] // 2 if d["gate"] else d["N"]) * d["G"])
    d.setdefault("ldr", 0 if d["res_bcast"] else (d["ldy"] if d["res_inplace"] else d["N"] * d["G"]))
    return d


def _rb(name, C, epi, T_out, routes=ALL6, B=3, wspread=False):
    """One batched ResBlock conv (k 3, dilation 3) in a rvcx_conv1d_gen epilogue (tests/test_gpu_conv_wst.py)."""
    kw = dict(B=B, T_in=T_out, C_in=C, N=C, taps=3, dil=3, pad=3, wspread=wspread)
    if epi in ("conv1", "prer"):
        kw.update(pre_act=LRELU, pre_slope=0.1)
    if epi == "conv1":
        kw.update(act=LRELU, slope=0.1)
    if epi in ("conv2", "acc", "accdiv", "prer"):
        kw.update(res="post")
    if epi in ("acc",):
        kw.update(acc=ACC_ADD)
    if epi in ("accdiv", "prer"):
        kw.update(acc=ACC_ADD_DIV, acc_div=3.0)
    return _c(name, "ResBlock convs batched (ADVICE r6; residuals.py:71-80)", routes, **kw)


# The rg.* rows' routes as rvcx_conv_plan admits them (admitted_routes below; tests/test_conv_form_ref_cpu.py holds the
# table to the planner): one input channel runs on the one-thread-per-output kernel alone, C_in = 16 and 80 are no
# multiple of the streamed kernels' 32-channel step, 3 steps are too few for the LDS-staged split, and the
# weight-stationary kernel takes none of these (7 or 11 taps, or C outside {64, 128}).
LDS3 = ("policy", "f32", "emu")
RG_ROUTES = {"rg.pre": ("policy",), "rg.down": LDS3, "rg.down_last": ALL5, "rg.cond": ALL5, "rg.mel": ALL5,
             "rg.up_in640": ALL5, "rg.up_in80": LDS3, "rg.rb_c1": ALL5, "rg.rb_c2": ALL5,
             "rg.rb32_c1": ("policy", "f32", "wsb", "gs")}

# the family the size policy picks per rg.* row (csrc/conv_dispatch.hip conv_plan at these shapes); every family a
# RefineGAN forward launches must be among them (tests/test_gpu_refinegan.py reads the launched families)
RG_POLICY = {"rg.pre": "conv_tiny_kernel", "rg.down": "conv_emu_kernel", "rg.down_last": "conv_gs16_kernel",
             "rg.cond": "conv_gs16_kernel", "rg.mel": "conv_gs16_kernel", "rg.up_in640": "conv_gs16_kernel",
             "rg.up_in80": "conv_emu_kernel", "rg.rb_c1": "conv_gs16_kernel", "rg.rb_c2": "conv_gs16_kernel",
             "rg.rb32_c1": "conv_gemm_kernel"}

CASES = [
    _c("te.emb_phone", "runtime_synth.cpp:639", ALL5, T_in=150, C_in=768, N=192, alpha=ALPHA192, res="pre",
       act=LRELU, slope=0.1, mask=True, flat=(75, 41)),
    _c("te.o_ln", "runtime_synth.cpp:667", ALL5, T_in=150, C_in=192, N=192, res="ln", res_inplace=True, ln=True),
    _c("te.ffn1", "runtime_synth.cpp:675", ALL5, B=2, T_in=70, C_in=192, N=768, taps=3, pad=1, pre_mask=True,
       lengths=(70, 41), act=RELU, wspread=True),
    _c("te.ffn2_ln", "runtime_synth.cpp:682", ALL5, B=2, T_in=70, C_in=768, N=192, taps=3, pad=1, pre_mask=True,
       mask=True, lengths=(70, 41), res="ln", res_inplace=True, ln=True),
    _c("te.proj", "runtime_synth.cpp:698", ALL5, T_in=140, C_in=192, N=384, pre_mask=True, mask=True, flat=(70, 41)),
    _c("flow.pre", "runtime_synth.cpp:768", ALL5, T_in=140, C_in=96, N=384, ldx=192, x_col0=96, mask=True,
       flat=(70, 41)),
    _c("flow.in_gate", "runtime_synth.cpp:775", ALL5, B=2, T_in=70, C_in=192, N=384, taps=5, pad=2, ldx=384,
       gate=True),
    _c("flow.rs_both", "runtime_synth.cpp:788", ALL5, T_in=140, C_in=192, N=384, acc=ACC_ADD, mask=True,
       flat=(70, 41)),
    _c("flow.rs_last", "runtime_synth.cpp:788", ALL5, T_in=140, C_in=192, N=192, ldy=384, y_col0=192, acc=ACC_ADD,
       mask=True, flat=(70, 41)),
    _c("flow.post", "runtime_synth.cpp:794", ALL5, T_in=140, C_in=192, N=96, ldx=384, x_col0=192, ldy=192,
       res="rsub", res_inplace=True, mask=True, flat=(70, 41)),
    _c("dec.pre", "runtime_synth.cpp:459", ALL5, B=2, T_in=70, C_in=192, N=512, taps=7, pad=3, pre_mask=True,
       lengths=(70, 41), res="pre", res_bcast=True),
    _c("dec.ups_nz", "runtime_synth.cpp:505", ("wsb", "wst"), B=2, T_in=100, T_out=100, C_in=64, N=64, taps=2, pad=1,
       pre_act=LRELU, pre_slope=0.1, nz=dict(u=2, C=32, stride=1)),
    _c("dec.ups_res", "runtime_synth.cpp:500", ALL6, B=2, T_in=100, T_out=100, C_in=128, N=128, taps=2, pad=1,
       pre_act=LRELU, pre_slope=0.1, res="post"),
    _c("dec.noise_pass", "runtime_synth.cpp:524", ("policy",), B=2, T_in=200, C_in=1, N=32, acc=ACC_ADD,
       wspread=True),
    _rb("rb128.conv1", 128, "conv1", 100),
    _rb("rb128.conv2", 128, "conv2", 100, wspread=True),
    _rb("rb64.acc", 64, "acc", 100),
    _rb("rb64.accdiv", 64, "accdiv", 100),
    _rb("rb64.prer", 64, "prer", 100),
    _rb("rb128.prer_long", 128, "prer", 25637),
    _c("hubert.conv_k3", "runtime_fe.cpp:155", ("policy", "f32", "emu", "gs"), B=2, T_in=301, C_in=512, N=512,
       taps=3, stride=2, act=GELU, bias=False),
    _c("hubert.conv_k2", "runtime_fe.cpp:155", ("policy", "f32", "emu", "gs"), B=2, T_in=301, C_in=512, N=512,
       taps=2, stride=2, act=GELU, bias=False),
    _c("hubert.pos_conv", "runtime_fe.cpp:175", ("policy", "f32", "emu"), B=2, G=16, T_in=49, T_out=49, C_in=48, N=48,
       taps=128, pad=64, act=GELU, res="post"),
    _c("hubert.ff1", "runtime_fe.cpp:233", ALL5, T_in=98, C_in=768, N=3072, act=GELU),
    _c("hubert.ff2_ln", "runtime_fe.cpp:239", ALL5, T_in=98, C_in=3072, N=768, res="ln", ln=True),
    _c("rm.stft", "runtime_fe.cpp:656", ("policy", "f32", "emu", "gs"), B=2, T_in=60, T_out=5, C_in=32, N=1026,
       taps=32, stride=5, bias=False),
    _c("rm.mel", "runtime_fe.cpp:671", ALL5, T_in=100, C_in=544, N=128, act=LOGCLAMP, slope=1e-5, bias=False,
       nonneg=True),
    _c("rm.fc", "runtime_fe.cpp:637", ALL5, T_in=100, C_in=512, N=360, act=SIGMOID),
    # The RefineGAN decoder's launch_conv sites (runtime_refinegan.cpp), forms no other site issues: one input channel
    # with unit row stride, the output written into the right half of the 512-wide concat, B entries of one row, C_in =
    # 80 (no multiple of 32), 11 taps at dilation 5 on a T_in barely past their 50-row reach, and the ResBlock's second
    # conv adding the buffer it writes (m = 1: r_in == dst). Routes: "policy" and every forced route rvcx_conv_plan
    # admits for the form (RG_REFUSED holds the others; test_gpu_conv_forms.py shows each one refused, not rerouted).
    _c("rg.pre", "runtime_refinegan.cpp:122", RG_ROUTES["rg.pre"], B=2, T_in=203, C_in=1, ldx=1, N=16, taps=7, pad=3),
    _c("rg.down", "runtime_refinegan.cpp:142", RG_ROUTES["rg.down"], B=2, T_in=101, C_in=16, N=32, taps=7, pad=3),
    _c("rg.down_last", "runtime_refinegan.cpp:142", RG_ROUTES["rg.down_last"], B=2, T_in=70, C_in=128, N=256, taps=7,
       pad=3, ldy=512, y_col0=256),
    _c("rg.cond", "runtime_refinegan.cpp:154", RG_ROUTES["rg.cond"], B=3, T_in=1, C_in=256, N=256),
    _c("rg.mel", "runtime_refinegan.cpp:162", RG_ROUTES["rg.mel"], B=2, T_in=70, C_in=192, N=256, taps=7, pad=3,
       pre_mask=True, lengths=(70, 41), res="pre", res_bcast=True, ldy=512),
    _c("rg.up_in640", "runtime_refinegan.cpp:195", RG_ROUTES["rg.up_in640"], B=2, T_in=70, C_in=640, N=256, taps=7,
       pad=3),
    _c("rg.up_in80", "runtime_refinegan.cpp:195", RG_ROUTES["rg.up_in80"], B=2, T_in=131, C_in=80, N=32, taps=7,
       pad=3),
    _c("rg.rb_c1", "runtime_refinegan.cpp:216", RG_ROUTES["rg.rb_c1"], B=2, T_in=60, C_in=64, N=64, taps=11, dil=5,
       pad=25, pre_act=LRELU, pre_slope=0.2, act=LRELU, slope=0.2),
    _c("rg.rb_c2", "runtime_refinegan.cpp:224", RG_ROUTES["rg.rb_c2"], B=2, T_in=60, C_in=64, N=64, taps=11, pad=5,
       res="post", res_inplace=True),
    _c("rg.rb32_c1", "runtime_refinegan.cpp:216", RG_ROUTES["rg.rb32_c1"], B=2, T_in=131, C_in=32, N=32, taps=3, dil=5,
       pad=5, pre_act=LRELU, pre_slope=0.2, act=LRELU, slope=0.2),
    # The edge forms of the LDS-staged families' shared gather (csrc/conv_lds.h), which no runtime site reaches (each
    # has C_in % 4 == 0 and 16-byte aligned rows): the scalar channel tail with a last chunk padded by zero channels
    # and a partial N tile, under a leaky-ReLU pre-activation and a row mask over non-zero rows (the mask applies to
    # the activated value); rows no vector load may touch (odd row stride, view one float in: the GEMM pipeline
    # unsplit, and its split over an odd number of chunks, which the LayerNorm forces); a strided dilated conv whose
    # halo reads before row 0 and past an odd T_in, with T_out a multiple of neither tile's rows.
    _c("lds.tail", "conv_lds.h lds_load4", ("f32", "emu"), B=2, T_in=150, C_in=50, N=40, taps=3, pad=1,
       pre_act=LRELU, pre_slope=0.1, pre_mask=True, lengths=(150, 113)),
    _c("lds.unaligned", "conv_lds.h lds_load4", ("f32", "emu"), B=2, T_in=70, C_in=64, N=64, ldx=65, x_col0=1),
    _c("lds.unaligned_split", "conv_lds.h lds_slice", ("f32", "emu"), T_in=70, C_in=96, N=64, ldx=97, x_col0=1,
       res="ln", ln=True),
    _c("lds.strided", "conv_lds.h lds_src_row", ("f32", "emu"), B=2, T_in=131, C_in=64, N=48, taps=3, stride=2, pad=1,
       dil=2),
]
BY_NAME = {c["name"]: c for c in CASES}


def linear(c):
    """Forms held to 1e-6 of the per-element magnitude sum (the others to K x the fp32 evaluation's own gap)."""
    return c["act"] in (NONE, LRELU, RELU) and not c["gate"] and not c["ln"]


def steps(c):
    return -(-c["C_in"] // 32) * c["taps"]


def tiny(c):
    """The same form at a size nested loops evaluate: every flag kept, the extents cut."""
    t = dict(c)
    T_out = min(c["T_out"], 7)
    t.update(C_in=min(c["C_in"], 3), taps=min(c["taps"], 3), G=min(c["G"], 2), T_out=T_out)
    t["N"] = 4 if (c["gate"] or c["nz"]) else min(c["N"], 5)
    if c["nz"]:
        t["nz"] = dict(u=2, C=2, stride=c["nz"]["stride"])
    t["pad"] = min(c["pad"], (t["taps"] - 1) * c["dil"])
    # keep the relation of T_out to the natural length (rm.stft and the ConvTranspose phases leave input rows unused)
    short = 1 if c["T_out"] < (c["T_in"] + 2 * c["pad"] - c["dil"] * (c["taps"] - 1) - 1) // c["stride"] + 1 else 0
    t_in = lambda: (T_out - 1) * c["stride"] + (t["taps"] - 1) * c["dil"] + 1 - 2 * t["pad"] + short  # noqa: E731
    if t_in() < 1:  # a "same" conv whose padding is half its reach (rg.rb_c1: dilation 5): full padding leaves no input
        t["pad"] = (t["taps"] - 1) * c["dil"] // 2
    t["T_in"] = t_in()
    if c["lengths"]:
        t["lengths"] = (t["T_in"], max(t["T_in"] - 3, 1))
    if c["flat"]:
        h = t["T_in"] // 2
        t["flat"] = (h, max(h - 2, 1))
        t["T_in"] = t["T_out"] = 2 * h
    return t


# ----------------------------------------------------------------- inputs
def _wspread(rng, N):
    """Per-column weight scales over 2^-12 .. 2^12 (tests/test_gpu_conv_wst.py "ch12")."""
    s = np.exp2(rng.integers(-12, 13, size=N)).astype(np.float64)
    s[0] = 2.0 ** 12
    s[min(5, N - 1)] = 2.0 ** -8
    return s


def _mask(c, T):
    if c["flat"]:
        per = c["flat"][0]
        assert T == per * len(c["flat"])
        return np.concatenate([(np.arange(per) < n) for n in c["flat"]]).astype(np.float32)[None]
    return np.stack([(np.arange(T) < min(n, T)) for n in c["lengths"]]).astype(np.float32)


def make(c):
    """Logical float32 arrays of a case (PCG64 seeded by the case name): masks hold zeros over non-zero data, a
    broadcast residual differs per batch entry."""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(c["name"].encode())))
    B, G, Ti, To, C, N, K = c["B"], c["G"], c["T_in"], c["T_out"], c["C_in"], c["N"], c["taps"]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    d = {"x": f(B, G, Ti, C), "w": (f(G, K, N, C) / np.float32(np.sqrt(C * K))).astype(np.float32)}
    d["bias"] = (0.1 * f(G, N)).astype(np.float32) if c["bias"] else None
    if c["nonneg"]:
        d["x"], d["w"] = np.abs(d["x"]), np.abs(d["w"])
        d["bias"] = None if d["bias"] is None else np.abs(d["bias"])
    if c["wspread"]:
        s = _wspread(rng, N)
        d["w"] = (d["w"] * s[None, None, :, None]).astype(np.float32)
        if d["bias"] is not None:
            d["bias"] = (d["bias"] * s[None]).astype(np.float32)
    d["res"] = None
    if c["res"]:
        d["res"] = f(B, 1, 1, N) if c["res_bcast"] else f(B, G, To, N)
    d["y0"] = f(B, G, To, N) if c["acc"] != ACC_STORE else None
    d["mask"] = _mask(c, To) if c["mask"] else None
    d["pre_mask"] = _mask(c, Ti) if c["pre_mask"] else None
    if c["gate"]:
        d["gate_g"] = f(B, N)
    if c["ln"]:
        d["ln_g"], d["ln_b"] = (1.0 + 0.2 * f(N)).astype(np.float32), (0.2 * f(N)).astype(np.float32)
    if c["nz"]:
        z = c["nz"]
        d["nz_har"] = f(B, To * z["u"] * z["stride"])
        d["nz_w"], d["nz_b"] = f(z["C"]), (0.1 * f(z["C"])).astype(np.float32)
    return d


# ----------------------------------------------------------------- the form
def _act(v, act, slope):
    if act == NONE:
        return v
    if act == LRELU:
        return torch.where(v > 0, v, v * slope)
    if act == RELU:
        return torch.clamp(v, min=0)
    if act == GELU:
        return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752440))
    if act == TANH:
        return torch.tanh(v)
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == LOGCLAMP:
        return torch.log(torch.clamp(v, min=slope))
    raise ValueError(act)


def _gelu_tanh(v):
    return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


def _contract(x, w, c):
    """x [B][G][T_in][C], w [G][K][N][C] -> [B][G][T_out][N]."""
    B, G = x.shape[0], x.shape[1]
    out = []
    for g in range(G):
        wg = w[g].permute(1, 2, 0)  # [N][C][K]
        y = torch.nn.functional.conv1d(x[:, g].transpose(1, 2), wg, None, stride=c["stride"], padding=c["pad"],
                                       dilation=c["dil"])
        out.append(y.transpose(1, 2)[:, :c["T_out"]])
    return torch.stack(out, 1)


def ref(d, c, dtype, mut=None):
    """The form of case c on the logical arrays d, evaluated in `dtype`. Returns (y [B][G][T_out][Ncol], mag): mag
    is the per-element magnitude sum (the same quantities in absolute value) for linear forms, else None. `mut` names
    a deviation (mutate's list) applied inside the evaluation."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    x, w, bias, R, y0, mask, pm = (t(d.get(k)) for k in ("x", "w", "bias", "res", "y0", "mask", "pre_mask"))
    lin = linear(c)
    xa = _act(x, c["pre_act"], c["pre_slope"])
    if pm is not None:
        xa = xa * pm[:, None, :, None]
    v = _contract(xa, w, c)
    mag = _contract(xa.abs(), w.abs(), c) if lin else None
    if bias is not None:
        v = v + bias[None, :, None, :]
        mag = mag + bias.abs()[None, :, None, :] if lin else None
    if c["gate"]:
        H = c["N"] // 2
        u = v + t(d["gate_g"])[:, None, None, :]
        a, b = (u[..., H:], u[..., :H]) if mut == "gate_swap" else (u[..., :H], u[..., H:])
        return torch.tanh(a) * torch.sigmoid(b), None
    res = {"pre": RES_ADD_PRE, "post": RES_ADD_POST, "rsub": RES_RSUB_POST}.get(c["res"], RES_NONE)
    if mut == "res_swap":
        res = {RES_ADD_PRE: RES_ADD_POST, RES_ADD_POST: RES_ADD_PRE, RES_RSUB_POST: RES_ADD_PRE}[res]
    alpha = c["alpha"]
    if mut == "alpha_before_res":
        v, mag, alpha = v * alpha, (mag * abs(alpha) if lin else None), 1.0
    if res == RES_ADD_PRE:
        v = v + R
        mag = mag + R.abs() if lin else None
    if alpha != 1.0 and mut != "alpha_after_act":
        v = v * alpha
        mag = mag * abs(alpha) if lin else None
    v = _gelu_tanh(v) if (mut == "gelu_tanh" and c["act"] == GELU) else _act(v, c["act"], c["slope"])
    if mut == "alpha_after_act":
        v = v * alpha
    if res == RES_ADD_POST:
        v = v + R
        mag = mag + R.abs() if lin else None
    elif res == RES_RSUB_POST:
        v = R - v
        mag = mag + R.abs() if lin else None
    if c["acc"] == ACC_ADD:
        v, mag = y0 + v, (y0.abs() + mag if lin else None)
    elif c["acc"] == ACC_ADD_DIV:
        div = 1.0 if mut == "acc_div" else c["acc_div"]
        v, mag = (y0 + v) / div, ((y0.abs() + mag) / c["acc_div"] if lin else None)
    if c["nz"]:
        z = c["nz"]
        B, To = v.shape[0], c["T_out"]
        har = t(d["nz_har"]).reshape(B, To, z["u"], z["stride"])[..., 0]  # [B][m][p]
        nw, nb = t(d["nz_w"]), t(d["nz_b"])
        nzv = (har[..., None] * nw + nb).reshape(B, 1, To, z["u"] * z["C"])
        v = v + nzv
        mag = mag + ((har.abs()[..., None] * nw.abs() + nb.abs()).reshape(B, 1, To, -1)) if lin else None
    if mask is not None:
        v = v * mask[:, None, :, None]
    if c["ln"]:
        r = R + v
        if mut == "ln_n1":  # the statistics over one column more (a zero), as a reduction one column too wide reads
            n1 = r.shape[-1] + 1
            mean = r.sum(-1, keepdim=True) / n1
            var = (((r - mean) ** 2).sum(-1, keepdim=True) + mean ** 2) / n1
        else:
            mean = r.mean(-1, keepdim=True)
            var = ((r - mean) ** 2).mean(-1, keepdim=True)
        return (r - mean) / torch.sqrt(var + c["ln_eps"]) * t(d["ln_g"]) + t(d["ln_b"]), None
    return v, mag


def ref_loops(d, c):
    """ref in float64 by nested loops over every output element (numpy scalars only): the independent statement."""
    import math

    def act(v, a, s):
        if a == LRELU:
            return v if v > 0 else v * s
        if a == RELU:
            return v if v > 0 else 0.0
        if a == GELU:
            return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))
        if a == TANH:
            return math.tanh(v)
        if a == SIGMOID:
            return 1.0 / (1.0 + math.exp(-v))
        if a == LOGCLAMP:
            return math.log(max(v, s))
        return v

    g = lambda k: None if d.get(k) is None else np.asarray(d[k], np.float64)  # noqa: E731
    x, w, bias, R, y0, mask, pm = (g(k) for k in ("x", "w", "bias", "res", "y0", "mask", "pre_mask"))
    B, G, To, N, C, K = c["B"], c["G"], c["T_out"], c["N"], c["C_in"], c["taps"]
    v = np.zeros((B, G, To, N))
    for b in range(B):
        for gi in range(G):
            for m in range(To):
                for n in range(N):
                    acc = 0.0
                    for k in range(K):
                        row = m * c["stride"] - c["pad"] + k * c["dil"]
                        if row < 0 or row >= c["T_in"]:
                            continue
                        for ch in range(C):
                            xv = act(x[b, gi, row, ch], c["pre_act"], c["pre_slope"])
                            if pm is not None:
                                xv *= pm[b, row]
                            acc += xv * w[gi, k, n, ch]
                    if bias is not None:
                        acc += bias[gi, n]
                    v[b, gi, m, n] = acc
    if c["gate"]:
        H = N // 2
        out = np.zeros((B, G, To, H))
        gg = g("gate_g")
        for b in range(B):
            for m in range(To):
                for h in range(H):
                    out[b, 0, m, h] = math.tanh(v[b, 0, m, h] + gg[b, h]) / (
                        1.0 + math.exp(-(v[b, 0, m, h + H] + gg[b, h + H])))
        return out
    out = np.zeros((B, G, To, N))
    for b in range(B):
        for gi in range(G):
            for m in range(To):
                for n in range(N):
                    e = v[b, gi, m, n]
                    r = None if R is None else (R[b, 0, 0, n] if c["res_bcast"] else R[b, gi, m, n])
                    if c["res"] == "pre":
                        e += r
                    e = act(e * c["alpha"], c["act"], c["slope"])
                    if c["res"] == "post":
                        e += r
                    elif c["res"] == "rsub":
                        e = r - e
                    if c["acc"] == ACC_ADD:
                        e = y0[b, gi, m, n] + e
                    elif c["acc"] == ACC_ADD_DIV:
                        e = (y0[b, gi, m, n] + e) / c["acc_div"]
                    if c["nz"]:
                        z = c["nz"]
                        p, ch = divmod(n, z["C"])
                        e += d["nz_w"][ch].astype(np.float64) * float(d["nz_har"][b, (m * z["u"] + p) * z["stride"]]) + float(
                            d["nz_b"][ch])
                    if mask is not None:
                        e *= mask[b, m]
                    out[b, gi, m, n] = e
            if c["ln"]:
                for m in range(To):
                    row = R[b, gi, m] + out[b, gi, m]
                    mean = sum(row) / N
                    var = sum((q - mean) ** 2 for q in row) / N
                    out[b, gi, m] = (row - mean) / math.sqrt(var + c["ln_eps"]) * g("ln_g") + g("ln_b")
    return out


# ----------------------------------------------------------------- deviations a wrong kernel could carry
MUTATIONS = ("mask_last_row", "pre_mask_first_row", "batch_offset", "alpha_after_act", "alpha_before_res", "res_swap",
             "acc_div", "guard_column", "ln_n1", "gate_swap", "gelu_tanh")


def applicable(c):
    """The mutations that change the value of case c (each must then be rejected). Left out where the mutated form is
    the same function: alpha after a positively homogeneous activation (leaky ReLU: te.emb_phone, the only runtime
    form with alpha; its alpha is probed by alpha_before_res instead), pre- and post-residual without an activation
    or alpha between them, a pre-mask whose rows the output mask zeroes anyway (one tap)."""
    m = ["guard_column"]
    if c["mask"]:
        m.append("mask_last_row")
    if c["pre_mask"] and (c["taps"] > 1 or not c["mask"]):
        m.append("pre_mask_first_row")
    if c["B"] > 1:
        m.append("batch_offset")
    if c["alpha"] != 1.0:
        if c["act"] not in (NONE, LRELU, RELU):
            m.append("alpha_after_act")
        if c["res"] == "pre":
            m.append("alpha_before_res")
    if c["res"] == "rsub" or (c["res"] in ("pre", "post") and (c["act"] != NONE or c["alpha"] != 1.0)):
        m.append("res_swap")
    if c["acc"] == ACC_ADD_DIV:
        m.append("acc_div")
    if c["ln"]:
        m.append("ln_n1")
    if c["gate"]:
        m.append("gate_swap")
    if c["act"] == GELU:
        m.append("gelu_tanh")
    return m


def mutate(d, c, mut):
    """-> (arrays, mut for ref): input-side deviations edit a copy of the arrays, the others are evaluated by ref."""
    d = dict(d)
    if mut == "mask_last_row":  # the mask not applied to the last row of each batch entry (a tile-edge row)
        mk = d["mask"].copy()
        if c["flat"]:
            per = c["flat"][0]
            mk[0, per - 1::per] = 1.0
        else:
            mk[:, -1] = 1.0
        assert not np.array_equal(mk, d["mask"]), "the mask must hold a zero on an entry's last row"
        d["mask"] = mk
        return d, None
    if mut == "pre_mask_first_row":  # the first masked input row of each entry let through
        pm = d["pre_mask"].copy()
        per = c["flat"][0] if c["flat"] else pm.shape[1]
        for i, n in enumerate(c["flat"] or c["lengths"]):
            if n < per:
                pm[(0, i * per + n) if c["flat"] else (i, n)] = 1.0
        assert not np.array_equal(pm, d["pre_mask"])
        d["pre_mask"] = pm
        return d, None
    if mut == "batch_offset":  # batch entry 1 read at entry 0's offset
        x = d["x"].copy()
        x[1] = x[0]
        d["x"] = x
        return d, None
    return d, mut


# ----------------------------------------------------------------- what the planner admits (host only)
# rvcx_conv1d_ex's route table (csrc/capi_test.cpp): the arithmetic, a static weight, the forced family, the family the
# launch has to get
ROUTE_PLAN = {"policy": (0, 1, None, None), "f32": (1, 0, None, "conv_gemm_kernel"), "emu": (2, 0, None, "conv_emu_kernel"),
              "wsb": (3, 1, "conv_wsb16_kernel", None), "gs": (3, 1, "conv_gs16_kernel", None),
              "wst": (3, 1, "conv_wst16_kernel", None)}


def admitted_routes(c, no_splitk=False):
    """{route: kernel family} for every route of rvcx_conv1d_ex that admits case c, asked of rvcx_conv_plan on the
    host (no context, no GPU) with the strides tests/test_gpu_conv_forms.py launches: a route is refused when no family
    admits the form under it or the family is not the route's own. Plain forms only (no gate, LayerNorm, noise)."""
    import ctypes

    from rvcx import _lib

    assert not (c["gate"] or c["ln"] or c["nz"] or c["G"] > 1)
    lib, L = _lib.load(), layout(c)
    kinds = {}
    for i in range(64):
        n = lib.rvcx_profile_kind_name(i)
        if n:
            kinds[n.decode()] = i
    out = {}
    for route, (math, stat, force, expect) in ROUTE_PLAN.items():
        d = _lib.ConvTestDesc()
        d.x, d.y, d.w = 0x100000 + 4 * c["x_col0"], 0x200000 + 4 * c["y_col0"], 0x300000  # read for alignment alone
        d.bias = 0x400000 if c["bias"] else None
        if c["res"]:
            d.res = d.y if c["res_inplace"] else 0x500000
            d.res_mode = {"pre": RES_ADD_PRE, "post": RES_ADD_POST, "rsub": RES_RSUB_POST}[c["res"]]
            d.ldr, d.res_bs = L["ldr"], L["res_bs"]
        if c["mask"]:
            d.mask, d.mask_bs = 0x600000, c["T_out"]
        if c["pre_mask"]:
            d.pre_mask, d.pre_mask_bs = 0x700000, c["T_in"]
        for k in ("T_in", "C_in", "N", "taps", "dil", "pad", "stride", "T_out", "pre_act", "act"):
            setattr(d, k, c[k])
        d.ldx, d.ldy, d.batch, d.batch_inner, d.x_bs, d.y_bs = L["ldx"], L["ldy"], c["B"], 1, L["x_bs"], L["y_bs"]
        d.pre_slope, d.slope, d.alpha, d.acc_div, d.acc_mode = c["pre_slope"], c["slope"], c["alpha"], c["acc_div"], c["acc"]
        d.no_splitk = 1 if no_splitk else 0
        got = [ctypes.c_int(-1) for _ in range(4)]
        rc = lib.rvcx_conv_plan(ctypes.byref(d), None, 0, stat, math, 0, kinds[force] if force else -1, -1,
                                *[ctypes.byref(o) for o in got])
        assert rc == 0, rc
        kind = next((n for n, i in kinds.items() if i == got[0].value), "other")
        if kind != "other" and (expect is None or kind == expect):
            out[route] = kind
    return out


# ----------------------------------------------------------------- strided buffers with guards
def extent(shape, ld, bs, bs2, col0=0):
    B, G, T, C = shape
    return col0 + (B - 1) * bs + (G - 1) * bs2 + (T - 1) * ld + C


def _index(shape, ld, bs, bs2, col0):
    B, G, T, C = shape
    b, g, t, ch = np.meshgrid(np.arange(B), np.arange(G), np.arange(T), np.arange(C), indexing="ij", sparse=True)
    return (col0 + b * bs + g * bs2 + t * ld + ch).reshape(-1)


def place(a, ld, bs, bs2, col0, total, fill):
    """Logical [B][G][T][C] -> (flat float32 buffer of `total` elements, valid mask): element (b, g, t, c) at
    col0 + b bs + g bs2 + t ld + c, every other element `fill` (a guard)."""
    buf = np.full(total, fill, np.float32)
    valid = np.zeros(total, bool)
    idx = _index(a.shape, ld, bs, bs2, col0)
    assert idx.max() < total and len(np.unique(idx)) == idx.size
    buf[idx] = np.asarray(a, np.float32).reshape(-1)
    valid[idx] = True
    return buf, valid


def gather(buf, shape, ld, bs, bs2, col0):
    return np.asarray(buf)[_index(shape, ld, bs, bs2, col0)].reshape(shape)


def guards_intact(after, before, valid):
    """Every element outside `valid` bit-identical to what it held before the launch."""
    a, b = np.asarray(after, np.float32).view(np.uint32), np.asarray(before, np.float32).view(np.uint32)
    return bool(np.array_equal(a[~valid], b[~valid]))


GAP_ROWS = 3  # guard rows between batch entries and after the last one


def layout(c):
    """Strides (floats) of a case's x / y / res buffers: rows of ld, G groups side by side in a row, batch entries
    GAP_ROWS guard rows apart."""
    L = {"ldx": c["ldx"], "ldy": c["ldy"], "ldr": c["ldr"], "x_bs2": c["C_in"] if c["G"] > 1 else 0,
         "y_bs2": c["N"] if c["G"] > 1 else 0, "res_bs2": c["N"] if c["G"] > 1 else 0}
    L["x_bs"] = (c["T_in"] + GAP_ROWS) * c["ldx"]
    L["y_bs"] = (c["T_out"] + GAP_ROWS) * c["ldy"]
    L["res_bs"] = c["N"] if c["res_bcast"] else (L["y_bs"] if c["res_inplace"] else (c["T_out"] + GAP_ROWS) * c["ldr"])
    L["x_total"] = c["B"] * L["x_bs"] + c["ldx"]
    L["y_total"] = c["B"] * L["y_bs"] + c["ldy"]
    L["res_total"] = c["B"] * L["res_bs"] + max(c["ldr"], c["N"])
    L["ycols"] = c["N"] // 2 if c["gate"] else c["N"]
    return L
