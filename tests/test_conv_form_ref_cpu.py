"""tests/conv_form_ref.py on the CPU: (a) its float64 statement of every form against nested loops over the output
elements at tiny extents, (b) every row of the case table is sensitive -- each deviation a wrong kernel could carry
(conv_form_ref.MUTATIONS), applied to the float64 reference on the very inputs tests/test_gpu_conv_forms.py uploads,
lands beyond the bar that file holds the device to (1e-6 of the element's magnitude sum for linear forms, K x the fp32
evaluation's own gap for the others) or trips its guard check. In the style of tests/test_parity_anchor_cpu.py.

Not applicable, by construction of the forms the runtime issues (conv_form_ref.applicable): alpha after the
activation (the one form with alpha, te.emb_phone, has a leaky ReLU, which commutes with a positive scale; its alpha is
probed by moving it before the pre-residual instead), pre- and post-residual swapped where neither activation nor
alpha stands between them.
"""
import numpy as np
import pytest
import torch

import conv_form_ref as cf
from parity_anchor import K, anchor, check

NAMES = [c["name"] for c in cf.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_ref_matches_nested_loops(name):
    c = cf.tiny(cf.BY_NAME[name])
    d = cf.make(c)
    y, mag = cf.ref(d, c, torch.float64)
    yl = cf.ref_loops(d, c)
    assert tuple(y.shape) == yl.shape
    err = float(np.abs(y.numpy() - yl).max())
    assert err <= 1e-12 * max(1.0, float(np.abs(yl).max())), err
    if cf.linear(c):
        assert mag is not None and bool((mag.numpy() >= np.abs(yl) * (1 - 1e-12)).all())
    else:
        assert mag is None


def test_inputs_hold_what_the_mutations_need():
    by = cf.BY_NAME
    assert by["te.emb_phone"]["alpha"] == float(np.float32(np.sqrt(192.0)))
    assert by["te.ffn1"]["lengths"] == (70, 41) and by["te.ffn2_ln"]["lengths"] == (70, 41)
    d = cf.make(by["dec.pre"])
    assert d["res"].shape == (2, 1, 1, 512) and not np.array_equal(d["res"][0], d["res"][1])
    for c in cf.CASES:
        d = cf.make(c)
        for k in ("mask", "pre_mask"):
            if d[k] is not None:  # zeros, over non-zero data, on the last row of some entry
                assert (d[k] == 0).any() and d[k].reshape(-1)[-1] == 0
                assert np.abs(d["x"]).min() > 0
    # per-column weight spread on at least one case of every kernel family (the routes of the spread cases)
    spread = [c for c in cf.CASES if c["wspread"]]
    assert {r for c in spread for r in c["routes"]} >= {"f32", "emu", "wsb", "gs", "wst"}
    assert by["dec.noise_pass"]["wspread"]  # the one-thread-per-output family


def _reject_value(c, y64, mag, anc, ym):
    """True when the device test's value bar refuses ym."""
    if cf.linear(c):
        return float((np.abs(ym - y64) / (mag + 1e-300)).max()) >= 1e-6
    try:
        check(c["name"], ym, anc[0], anc[1], K)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", NAMES)
def test_case_is_sensitive(name):
    c = cf.BY_NAME[name]
    d = cf.make(c)
    y64, mag = cf.ref(d, c, torch.float64)
    y64 = y64.numpy()
    mag = None if mag is None else mag.numpy()
    anc = None if cf.linear(c) else anchor(lambda dt: cf.ref(d, c, dt)[0])["out"]
    assert not _reject_value(c, y64, mag, anc, y64)
    muts = cf.applicable(c)
    print(f"\n{name}: mutations {muts}")
    survived = []
    for m in muts:
        if m == "guard_column":
            L = cf.layout(c)
            shape = (c["B"], c["G"], c["T_out"], L["ycols"])
            before, valid = cf.place(np.zeros(shape, np.float32), L["ldy"], L["y_bs"], L["y_bs2"], c["y_col0"],
                                     L["y_total"], cf.SENTINEL)
            assert (~valid).any(), "no guard element"
            after = before.copy()
            assert cf.guards_intact(after, before, valid)
            g = np.flatnonzero(~valid)
            for at in (g[0], g[len(g) // 2], g[-1]):
                after = before.copy()
                after[at] = 0.0
                if cf.guards_intact(after, before, valid):
                    survived.append(m)
            continue
        dm, mm = cf.mutate(d, c, m)
        ym = cf.ref(dm, c, torch.float64, mm)[0].numpy()
        if not _reject_value(c, y64, mag, anc, ym):
            survived.append(m)
    assert not survived, f"{name}: not rejected: {survived}"


RG = [c["name"] for c in cf.CASES if c["name"].startswith("rg.")]
RG_POLICY = cf.RG_POLICY


@pytest.mark.parametrize("name", RG)
def test_refinegan_rows_list_the_routes_the_planner_admits(name):
    """The rg.* rows (runtime_refinegan.cpp's launch_conv sites): the row's route list is exactly what rvcx_conv_plan
    admits for its form, with and without split-K, and the policy's family is the recorded one."""
    c = cf.BY_NAME[name]
    assert c["site"].startswith("runtime_refinegan.cpp:")
    for nsk in (False, True):
        adm = cf.admitted_routes(c, nsk)
        assert tuple(r for r in cf.ALL6 if r in adm) == c["routes"], (name, nsk, adm)
        assert adm["policy"] == RG_POLICY[name], adm
    print(f"\n{name} [{c['site']}]: policy -> {RG_POLICY[name]}; refused: "
          f"{[r for r in cf.ALL6 if r not in c['routes']]}")


def test_refinegan_rows_cover_every_launch_conv_site():
    """Every launch_conv call of csrc/runtime_refinegan.cpp is cited by at least one rg.* row, by its line."""
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "retrieval-based-voice-conversion-mlx_amd", "csrc", "runtime_refinegan.cpp")
    sites = {i + 1 for i, line in enumerate(open(src)) if re.search(r"\blaunch_conv\(", line)}
    cited = {int(cf.BY_NAME[n]["site"].split(":")[1]) for n in RG}
    assert sites and sites == cited, (sorted(sites), sorted(cited))
    assert set(RG_POLICY) == set(RG)


def test_every_listed_mutation_is_applied_somewhere():
    used = {m for c in cf.CASES for m in cf.applicable(c)}
    assert used == set(cf.MUTATIONS) - {"alpha_after_act"}, sorted(set(cf.MUTATIONS) - used)


def test_alpha_after_act_is_visible_where_the_activation_does_not_commute():
    """The listed alpha mutation on a form of its own (alpha with GELU: not a runtime form), so that the mutation's
    code is exercised; on te.emb_phone it is the identity up to rounding."""
    c = dict(cf.tiny(cf.BY_NAME["te.emb_phone"]), act=cf.GELU)
    d = cf.make(c)
    assert "alpha_after_act" in cf.applicable(c)
    y = cf.ref(d, c, torch.float64)[0]
    ym = cf.ref(d, c, torch.float64, "alpha_after_act")[0]
    assert float((y - ym).abs().max()) > 1e-3
    c = cf.tiny(cf.BY_NAME["te.emb_phone"])
    y = cf.ref(d, c, torch.float64)[0]
    ym = cf.ref(d, c, torch.float64, "alpha_after_act")[0]
    assert float((y - ym).abs().max()) < 1e-12
