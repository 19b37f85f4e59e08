"""The conv planner against the recorded routing table (tests/golden/conv_routes.json, its rows in conv_routes.npz).
No GPU.

The table holds one row per distinct conv launch of the whole GPU suite and of one bench.py step of every configuration,
recorded on the commit before conv_plan existed: the launch's form and what the old dispatcher chain ran (family, tile,
ksplit, weight image). rvcx_conv_plan (include/rvcx_test.h), fed each row's form, has to return exactly that: a rule
that moved into the planner changed no launch.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from rvcx import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
# ConvKind (csrc/conv_kernels.h)
CK_WSB16, CK_WSB, CK_GS, CK_GSW, CK_RBPAIR, CK_SMALL2D, CK_EMU, CK_GEMM, CK_TINY, CK_WST, CK_OTHER = range(11)
# what a conv launch can produce: not the fused ResBlock pair (its own launcher), not "other", and not conv_wsb_kernel
# (the bf16 32x32x16 form, which no longer exists)
LAUNCHABLE = {CK_WSB16, CK_GS, CK_GSW, CK_SMALL2D, CK_EMU, CK_GEMM, CK_TINY, CK_WST}
WSB_TILES = {23, 24, 25, 27}


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        doc = json.load(f)
    rows = np.load(TABLE[:-5] + ".npz", allow_pickle=False)["rows"]
    cols = doc["columns"]
    # the matrix the descriptor names: every recorded row, none left out
    assert rows.dtype == np.int32 and rows.shape == (doc["n_rows"], len(cols))
    assert hashlib.sha256(rows.tobytes()).hexdigest() == doc["rows_sha256"]
    return [dict(doc["constants"], **dict(zip(cols, r))) for r in rows.tolist()]


def _ptr(mod16):
    """A recorded pointer: null (-1) or any address with that remainder modulo 16."""
    return None if mod16 < 0 else 0x10000 + mod16


def plan(lib, r):
    d = _lib.ConvTestDesc()
    d.x, d.y, d.w, d.res = _ptr(r["x16"]), _ptr(r["y16"]), _ptr(r["w16"]), _ptr(r["res16"] if r["res"] else -1)
    for name in ("bias", "mask", "pre_mask", "ln_g"):
        setattr(d, name, _ptr(0 if r[name] else -1))
    d.ln_b, d.gate_g = d.ln_g, _ptr(0 if r["gate_h"] else -1)
    d.nz_har = d.nz_w = d.nz_b = _ptr(0 if r["nz"] else -1)
    for k in ("T_in", "C_in", "N", "taps", "dil", "pad", "stride", "T_out", "ldx", "ldy", "ldr", "batch", "batch_inner",
              "pre_act", "act", "res_mode", "acc_mode", "gate_h", "nz_stride", "nz_kk", "nz_u", "nz_C", "no_splitk"):
        setattr(d, k, r[k])
    d.x_bs, d.y_bs, d.res_bs = r["x_bs4"], r["y_bs4"], r["res_bs4"]
    d.alpha, d.acc_div = (1.0 if r["alpha1"] else 2.0), 1.0
    f = _lib.ConvPlanForm()
    for k in ("W_in", "W_out", "KH", "KW", "padh", "padw", "out_map", "out_cv", "lowp", "ldw", "w_bs", "bias_bs"):
        setattr(f, k, r[k])
    f.w_ts = 4 * r["N"] * r["ldw"] + r["w_ts4"]  # any tap stride with the recorded remainder modulo 4
    out = [ctypes.c_int(-99) for _ in range(4)]
    rc = lib.rvcx_conv_plan(ctypes.byref(d), ctypes.byref(f), r["two_d"], r["stat"], r["math"], r["plan_T"],
                            r["force_kind"], r["force_tile"], *[ctypes.byref(o) for o in out])
    assert rc == 0
    return tuple(o.value for o in out)


def test_table_covers_the_dispatcher(table):
    kinds = {r["kind"] for r in table}
    assert kinds == LAUNCHABLE, sorted(LAUNCHABLE ^ kinds)
    split = {r["kind"] for r in table if r["ksplit"] > 1}
    assert split >= {CK_GS, CK_GSW, CK_WSB16, CK_EMU, CK_GEMM}, split
    assert any(r["plan_T"] > r["T_out"] for r in table)
    assert {r["tile"] for r in table if r["kind"] == CK_WSB16} == WSB_TILES
    # the launches the old chain handed on after a launcher refused: the reduced-precision ones of gather-streamed shapes
    fell = [r for r in table if r["fell"]]
    assert fell and all(r["lowp"] and r["kind"] == CK_EMU for r in fell)
    assert any(r["force_kind"] >= 0 for r in table) and any(r["two_d"] for r in table)


def test_planner_reproduces_every_recorded_launch(table):
    lib = _lib.load()
    bad = []
    for i, r in enumerate(table):
        got, want = plan(lib, r), (r["kind"], r["tile"], r["ksplit"], r["fmt"])
        if got != want:
            bad.append((i, got, want, {k: r[k] for k in ("two_d", "stat", "math", "plan_T", "force_kind", "force_tile",
                                                          "C_in", "N", "taps", "T_out", "W_out", "batch", "lowp")}))
    assert not bad, f"{len(bad)} of {len(table)} rows differ, e.g. {bad[:5]}"
