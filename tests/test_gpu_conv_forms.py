"""Every 1-D contraction form the runtime issues, at kernel level against float64 (rvcx_conv1d_ex).

The case table (tests/conv_form_ref.py CASES, one row per runtime call site, the line cited per row) runs under the
size policy (route "policy": kind and split count printed) and under every forced route that admits the form: exact
fp32 MFMA ("f32"), the LDS-staged bf16 split ("emu"), the weight-streamed tile ("wsb"), gather-streamed ("gs"),
weight-stationary ("wst"); contractions of more than 3 steps with split-K allowed and with no_splitk. Per launch:

    ran where it says   a forced route reports its own family; the union over the table covers every 1-D family
    value               linear forms (no activation, leaky ReLU, ReLU; no gate, no LayerNorm): every element within 1e-6
                        of its own magnitude sum of float64 (the bar of test_gpu_conv_math.py / test_gpu_conv_wst.py);
                        the others within K = 8 x the float32 CPU evaluation's own distance to float64 on the same
                        inputs (tests/parity_anchor.py)
    guards              output: columns [N, ldy), the untouched half rows, the rows past T_out and between batch
                        entries hold a sentinel bit pattern and must keep it; input: everything outside the view is NaN
                        and the output must stay finite
    batch independence  forced route, no_splitk: each entry of a B > 1 launch equals the B = 1 launch of that entry, bit
                        for bit (the gate and LayerNorm forms cannot: they always split, and the split count follows the
                        batch size)
    kernel identity     weight-stationary == weight-streamed bit for bit; the fused noise conv == a separate
                        accumulate pass

tests/test_conv_form_ref_cpu.py shows, without a GPU, that each row's inputs make these assertions sensitive.
"""
import functools

import numpy as np
import pytest
import torch

import conv_form_ref as cf
from parity_anchor import K, anchor, check

pytestmark = pytest.mark.gpu

KIND = {"f32": "conv_gemm_kernel", "emu": "conv_emu_kernel", "wsb": "conv_wsb16_kernel", "gs": "conv_gs16_kernel",
        "wst": "conv_wst16_kernel"}
FAMILIES = set(KIND.values()) | {"conv_tiny_kernel"}  # every 1-D family the dispatcher can report
E_SHAPE = -2
SEEN = {}  # (case, route, no_splitk) -> (kind, ksplit)


def _params():
    out = []
    for c in cf.CASES:
        combine = c["gate"] or c["ln"]
        for r in c["routes"]:
            # no_splitk on and off where the contraction has more than 3 steps and the route can split at all
            both = cf.steps(c) > 3 and not combine and r != "wst"
            for nsk in ((False, True) if both else ((False,) if combine or r == "policy" else (True,))):
                out.append(pytest.param(c["name"], r, nsk, id=f"{c['name']}-{r}-{'nosplit' if nsk else 'split'}"))
    return out


@functools.lru_cache(maxsize=2)
def _reference(name):
    c = cf.BY_NAME[name]
    d = cf.make(c)
    if cf.linear(c):
        y, mag = cf.ref(d, c, torch.float64)
        return d, y.numpy(), mag.numpy(), None
    y, gap = anchor(lambda dt: cf.ref(d, c, dt)[0])["out"]
    return d, y, None, gap


class Buffers:
    """A case's operands on the device, strided as the runtime holds them, every element outside a view a guard."""

    def __init__(self, engine, c, d=None):
        self.c, self.L = c, cf.layout(c)
        d = cf.make(c) if d is None else d
        L, dev = self.L, engine.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
        x, _ = cf.place(d["x"], L["ldx"], L["x_bs"], L["x_bs2"], c["x_col0"], L["x_total"], np.nan)
        self.x = up(x)
        self.w = up(d["w"].reshape(-1))
        self.bias = None if d["bias"] is None else up(d["bias"].reshape(-1))
        self.res = None
        shape = (c["B"], c["G"], c["T_out"], L["ycols"])
        init = np.full(shape, cf.SENTINEL, np.float32)
        if c["acc"] != cf.ACC_STORE:
            init = d["y0"]
        if c["res"] and c["res_inplace"]:
            init = d["res"]
        elif c["res"]:
            ld = c["N"] if c["res_bcast"] else L["ldr"]
            r, _ = cf.place(d["res"], ld, L["res_bs"], L["res_bs2"], 0, L["res_total"], np.nan)
            self.res = up(r)
        self.y_init, self.valid = cf.place(init, L["ldy"], L["y_bs"], L["y_bs2"], c["y_col0"], L["y_total"],
                                           cf.SENTINEL)
        self.mask = None if d["mask"] is None else up(d["mask"].reshape(-1))
        self.pre_mask = None if d["pre_mask"] is None else up(d["pre_mask"].reshape(-1))
        self.gate_g = up(d["gate_g"].reshape(-1)) if c["gate"] else None
        self.ln_g, self.ln_b = (up(d["ln_g"]), up(d["ln_b"])) if c["ln"] else (None, None)
        if c["nz"]:
            n = d["nz_har"].shape[1]
            self.nz_bs = n + 5
            h = np.full((c["B"], self.nz_bs), np.nan, np.float32)
            h[:, :n] = d["nz_har"]
            self.nz_har, self.nz_w, self.nz_b = up(h.reshape(-1)), up(d["nz_w"]), up(d["nz_b"])
        self.dev = dev

    def launch(self, engine, route, nsk, entry=None, y=None, **over):
        """One launch into a fresh copy of the initial output buffer (or into `y`); entry = b runs batch entry b
        alone as a B = 1 launch on the same memory. Returns (the whole output buffer, kind, ksplit)."""
        c, L = self.c, self.L
        yb = torch.from_numpy(self.y_init).to(self.dev) if y is None else y
        off = (lambda bs: 0) if entry is None else (lambda bs: entry * bs)
        cut = lambda t, o: None if t is None else t[o:]  # noqa: E731
        G = c["G"]
        kw = dict(x=self.x[c["x_col0"] + off(L["x_bs"]):], w=self.w, y=yb[c["y_col0"] + off(L["y_bs"]):],
                  bias=self.bias, T_in=c["T_in"], C_in=c["C_in"], N=c["N"], T_out=c["T_out"], ldx=L["ldx"], ldy=L["ldy"],
                  taps=c["taps"], dil=c["dil"], pad=c["pad"], stride=c["stride"],
                  batch=c["B"] if entry is None else 1, x_bs=L["x_bs"], y_bs=L["y_bs"], batch_inner=G,
                  x_bs2=L["x_bs2"], y_bs2=L["y_bs2"], w_bs2=c["taps"] * c["N"] * c["C_in"] if G > 1 else 0,
                  bias_bs2=c["N"] if G > 1 else 0, pre_act=c["pre_act"], pre_slope=c["pre_slope"], act=c["act"],
                  slope=c["slope"], alpha=c["alpha"], acc_mode=c["acc"], acc_div=c["acc_div"], route=route,
                  no_splitk=nsk)
        if c["res"]:
            kw.update(res=kw["y"] if c["res_inplace"] else self.res[off(L["res_bs"]):], ldr=L["ldr"],
                      res_bs=L["res_bs"], res_bs2=L["res_bs2"],
                      res_mode={"pre": cf.RES_ADD_PRE, "post": cf.RES_ADD_POST, "rsub": cf.RES_RSUB_POST,
                                "ln": cf.RES_NONE}[c["res"]])
        if c["mask"]:
            kw.update(mask=cut(self.mask, off(c["T_out"])), mask_bs=c["T_out"])
        if c["pre_mask"]:
            kw.update(pre_mask=cut(self.pre_mask, off(c["T_in"])), pre_mask_bs=c["T_in"])
        if c["gate"]:
            kw.update(gate_h=c["N"] // 2, gate_g=cut(self.gate_g, off(c["N"])), gate_g_bs=c["N"])
        if c["ln"]:
            kw.update(ln_g=self.ln_g, ln_b=self.ln_b, ln_eps=c["ln_eps"])
        if c["nz"]:
            z = c["nz"]
            kw.update(nz_har=cut(self.nz_har, off(self.nz_bs)), nz_bs=self.nz_bs, nz_stride=z["stride"], nz_kk=1,
                      nz_u=z["u"], nz_C=z["C"], nz_w=self.nz_w, nz_b=self.nz_b)
        kw.update(over)
        _, kind, ksplit = engine.conv1d_ex(**kw)
        return yb, kind, ksplit

    def values(self, ybuf):
        c, L = self.c, self.L
        return cf.gather(ybuf, (c["B"], c["G"], c["T_out"], L["ycols"]), L["ldy"], L["y_bs"], L["y_bs2"], c["y_col0"])


@functools.lru_cache(maxsize=2)
def _buffers(engine, name):
    return Buffers(engine, cf.BY_NAME[name], _reference(name)[0])


def _run(engine, name, route, nsk):
    yb, kind, ksplit = _buffers(engine, name).launch(engine, route, nsk)
    SEEN[(name, route, nsk)] = (kind, ksplit)
    return engine.host(yb), kind, ksplit


@pytest.mark.parametrize("name,route,nsk", _params())
def test_form(engine, name, route, nsk):
    c = cf.BY_NAME[name]
    d, y64, mag, gap = _reference(name)
    bufs = _buffers(engine, name)
    after, kind, ksplit = _run(engine, name, route, nsk)
    if route != "policy":
        assert kind == KIND[route], (kind, route)
    else:  # the launch ran what the planner, asked on the host alone, says it decides for this descriptor
        pk, _, pks, _ = engine.conv_plan()
        assert (kind, ksplit) == (pk, pks), (kind, ksplit, pk, pks)
    assert kind in FAMILIES, kind
    assert ksplit >= 1 and (ksplit == 1 or not nsk)
    if c["gate"] or c["ln"]:
        assert ksplit >= 2  # the combine kernels are where these epilogues live
    y = bufs.values(after)
    assert np.isfinite(y).all(), f"{name}: non-finite output (a NaN input guard was read)"
    if cf.linear(c):
        err, bound = float((np.abs(y - y64) / (mag + 1e-300)).max()), 1e-6
    else:
        scale = float(np.abs(y64).max())
        err, bound = float(np.abs(y - y64).max()) / scale, K * max(gap / scale, 2.0 ** -23)
    print(f"\n{name} [{c['site']}] {route}{' no_splitk' if nsk else ''}: {kind} ksplit {ksplit} err {err:.3e} "
          f"bound {bound:.3e}")
    if cf.linear(c):
        assert err < bound, (name, route, err)
    else:
        check(f"{name} {route}", y, y64, gap, K)
    assert cf.guards_intact(after, bufs.y_init, bufs.valid), f"{name}: an output guard element was written"


BATCHED = [(c["name"], r) for c in cf.CASES if c["B"] > 1 and not (c["gate"] or c["ln"])
           for r in c["routes"] if r != "policy"]


@pytest.mark.parametrize("name,route", BATCHED, ids=[f"{n}-{r}" for n, r in BATCHED])
def test_batch_entry_equals_single_launch(engine, name, route):
    c = cf.BY_NAME[name]
    bufs = _buffers(engine, name)
    whole, kind, _ = bufs.launch(engine, route, True)
    whole = bufs.values(engine.host(whole))
    for b in range(c["B"]):
        one, k1, _ = bufs.launch(engine, route, True, entry=b)
        assert k1 == kind == KIND[route]
        one = bufs.values(engine.host(one))
        assert np.array_equal(one[b], whole[b]), (name, route, b, float(np.abs(one[b] - whole[b]).max()))


BOTH = [c["name"] for c in cf.CASES if "wsb" in c["routes"] and "wst" in c["routes"]]


@pytest.mark.parametrize("name", BOTH)
def test_wst_equals_wsb(engine, name):
    """the weight-stationary kernel's tile cursor wraps from one batch entry to the next inside a persistent
    run; every element of every entry must equal the weight-streamed kernel's (rb128.prer_long: 401 tiles per entry,
    1203 in all, more than the grid, runs of 3 or 5 straddling the entry boundaries)."""
    a, ka, _ = _run(engine, name, "wst", True)
    b, kb, _ = _run(engine, name, "wsb", True)
    assert (ka, kb) == (KIND["wst"], KIND["wsb"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), float(np.nanmax(np.abs(a - b)))


@pytest.mark.parametrize("route", ["wsb", "wst"])
def test_fused_noise_equals_separate_pass(engine, route):
    """dec.ups with the noise conv in its epilogue (runtime_synth.cpp:505) == the same launch without it followed by
    the one-tap noise conv as an ACC_ADD pass over y as [T u][C] (runtime_synth.cpp:524), bit for bit."""
    c = cf.BY_NAME["dec.ups_nz"]
    d = cf.make(c)
    fused, kind, _ = Buffers(engine, c, d).launch(engine, route, True)
    plain = dict(c, nz=None)
    pb = Buffers(engine, plain, d)
    y, _, _ = pb.launch(engine, route, True)
    z, L = c["nz"], cf.layout(c)
    rows = c["T_out"] * z["u"]
    har = torch.full((c["B"], rows + 5), float("nan"), device=engine.device)
    har[:, :rows] = torch.from_numpy(d["nz_har"]).to(engine.device)
    nw, nb = (torch.from_numpy(d[k]).to(engine.device) for k in ("nz_w", "nz_b"))
    _, k2, _ = engine.conv1d_ex(x=har.reshape(-1), w=nw, y=y, bias=nb, T_in=rows, C_in=1, N=z["C"], T_out=rows, ldx=1,
                                ldy=z["C"], batch=c["B"], x_bs=rows + 5, y_bs=L["y_bs"], acc_mode=cf.ACC_ADD,
                                route="policy")
    assert (kind, k2) == (KIND[route], "conv_tiny_kernel")
    a, b = engine.host(fused), engine.host(y)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), float(np.nanmax(np.abs(a - b)))


def _refused(engine, c, route, **over):
    from rvcx._lib import RvcxError

    bufs = Buffers(engine, c)
    y = torch.from_numpy(bufs.y_init).to(engine.device)
    with pytest.raises(RvcxError) as e:
        bufs.launch(engine, route, over.pop("nsk", False), y=y, **over)
    assert e.value.code == E_SHAPE, str(e.value)
    assert np.array_equal(engine.host(y).view(np.uint32), bufs.y_init.view(np.uint32)), "y written by a refused call"


def _case(**kw):
    base = dict(T_in=40, C_in=128, N=128, taps=3, pad=1)
    base.update(kw)
    return cf._c("refusal", "-", (), **base)


@pytest.mark.parametrize("what", ["mask", "pre_mask", "alpha"])
def test_weight_stationary_refuses_masks_and_alpha(engine, what):
    kw = dict(alpha=2.0) if what == "alpha" else {what: True, "lengths": (33,)}
    _refused(engine, _case(**kw), "wst", nsk=True)
    _refused(engine, _case(), "wst", nsk=True, act=cf.GELU)  # nor an activation its epilogue lacks


@pytest.mark.parametrize("route", ["policy", "f32", "emu", "wsb", "gs"])
def test_combine_epilogues_refuse_what_the_combine_cannot_do(engine, route):
    ln = dict(res="ln", res_inplace=True, ln=True)
    _refused(engine, _case(C_in=192, N=1025, taps=1, pad=0, **ln), route)            # LN wider than one block's 1024
    _refused(engine, _case(C_in=32, N=128, taps=1, pad=0, **ln), route)              # one step: nothing to split
    _refused(engine, _case(C_in=32, N=128, taps=1, pad=0, gate=True), route)
    _refused(engine, _case(C_in=192, N=128, taps=1, pad=0, **ln), route, nsk=True)   # no_splitk leaves no combine
    _refused(engine, _case(C_in=192, N=128, taps=1, pad=0, gate=True), route, gate_h=48)  # N != 2 gate_h


def test_forced_routes_refuse_foreign_shapes(engine):
    """A forced route never runs on another kernel: strided and grouped forms under the streamed kernels, a
    one-thread-per-output shape under the MFMA kernels, the fused noise conv where the policy would not stream the
    weights (the runtime fuses it only where conv_routes_wsb16 holds: at T = 100 the policy picks the gather-streamed
    kernel, which has no noise epilogue)."""
    by = cf.BY_NAME
    _refused(engine, by["hubert.conv_k3"], "wsb", nsk=True)
    _refused(engine, by["hubert.pos_conv"], "gs", nsk=True)
    _refused(engine, by["hubert.pos_conv"], "wsb", nsk=True)
    _refused(engine, by["rm.stft"], "wst", nsk=True)
    for r in ("f32", "emu", "wsb", "gs", "wst"):
        _refused(engine, by["dec.noise_pass"], r, nsk=True)
    _refused(engine, by["dec.ups_nz"], "policy", nsk=True)
    _refused(engine, by["dec.ups_nz"], "gs", nsk=True)
    _refused(engine, by["dec.ups_nz"], "emu", nsk=True)


RG_REFUSED = [(c["name"], r) for c in cf.CASES if c["name"].startswith("rg.") for r in cf.ALL6 if r not in c["routes"]]


@pytest.mark.parametrize("name,route", RG_REFUSED, ids=[f"{n}-{r}" for n, r in RG_REFUSED])
def test_refinegan_rows_refused_routes_are_refused(engine, name, route):
    """The routes rvcx_conv_plan does not admit for an rg.* row (tests/test_conv_form_ref_cpu.py holds the lists to the
    planner): RVCX_E_SHAPE, nothing written, never another kernel."""
    _refused(engine, cf.BY_NAME[name], route, nsk=True)


def test_every_family_is_reached(engine):
    """Runs last. The union of the kinds the table reported covers every 1-D family of ConvKind (conv_wsb_kernel, the
    bf16 32x32x16 form, no longer exists; k_rb_pair and the 2-D families are not conv1d's), the policy alone reaches
    each family the runtime uses, and all three combine kernels ran (plain, gate, LayerNorm: a split launch of each)."""
    for p in _params():  # whatever a deselection left out (launch only)
        name, route, nsk = p.values
        if (name, route, nsk) not in SEEN:
            _run(engine, name, route, nsk)
    kinds = {k for k, _ in SEEN.values()}
    assert kinds == FAMILIES, sorted(FAMILIES - kinds)
    policy = {k for (n, r, s), (k, _) in SEEN.items() if r == "policy"}
    print(f"\npolicy kinds: {sorted(policy)}")
    assert policy >= {"conv_wst16_kernel", "conv_gs16_kernel", "conv_emu_kernel", "conv_tiny_kernel"}, policy
    split = {n for (n, r, s), (k, ks) in SEEN.items() if ks > 1}
    by = cf.BY_NAME
    assert any(by[n]["gate"] for n in split) and any(by[n]["ln"] for n in split)
    assert any(not by[n]["gate"] and not by[n]["ln"] for n in split)
