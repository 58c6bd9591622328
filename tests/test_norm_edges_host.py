"""CPU half of the normalisation / pointwise edge tests: the input families of tests/_norm_cases.py have their stated property at
every shape the GPU tests use, every reference is finite and the fp32 reference's own error stays below 1e-4 under the metric (so
the bound `M x that error` can hide nothing), every variant's shape reaches the launch plan it is listed for (the library's host
queries and the restated plans agree), and the supported / refused edges sit where the kernels' launchers put them.  Nothing here
touches a kernel."""
import types

import pytest
import torch

import _norm_cases as A

GN_CASES = [(v, f) for v in A.GN_VARIANTS for f in v["families"]]
LN_CASES = [(v, f) for v in A.LN_VARIANTS for f in v["families"]]
GEGLU_CASES = [(v, g, s) for v in A.GEGLU_VARIANTS for g, s in v["cases"]]


@pytest.fixture(scope="module")
def lib():
    from stablekeypoints_amd import _native
    return _native.lib()


@pytest.mark.parametrize("v,family", GN_CASES, ids=[f"{v['name']}-{f}" for v, f in GN_CASES])
def test_group_norm_family_property_and_reference_error(v, family):
    c = A.gn_case(v, family)
    G = v["shape"][2]
    ok, what = A.check_property("gn", family, c.x, G)
    assert ok, f"{c.what}: {what}"
    if c.dy is not None:
        ok, what_dy = A.check_property("dy", c.dy_family, c.dy, G)
        assert ok, f"{c.what} dy {c.dy_family}: {what_dy}"
    if family == "saturating" and v["kind"] != "coef":
        off = 0 if c.off is None else c.off.double()[:, :, None, None]
        z = torch.nn.functional.group_norm(c.x.double() + off, G, c.gamma.double(), c.beta.double(), v["eps"])
        assert z.max().item() > 88.8 and z.min().item() < -88.8, "z does not pass the overflow of exp() in fp32"
    found = A.input_conditions(c)
    print(f"{c.what}: {what}; fp32 reference " + ", ".join(f"{k} {e:.1e}" for k, e in found.items()))


@pytest.mark.parametrize("v,family", LN_CASES, ids=[f"{v['name']}-{f}" for v, f in LN_CASES])
def test_layer_norm_family_property_and_reference_error(v, family):
    c = A.ln_case(v, family)
    exact = c.h.double() if c.d is None else c.d.double() + c.h.double()
    ok, what = A.check_property("ln", family, exact, aux=(c.d, c.h))
    assert ok, f"{c.what}: {what}"
    assert (c.d is not None) == (v["with_d"] or family == "cancelling")
    found = A.input_conditions(c)
    print(f"{c.what}: {what}; fp32 reference " + ", ".join(f"{k} {e:.1e}" for k, e in found.items()))


@pytest.mark.parametrize("v,gates,hscale", GEGLU_CASES, ids=[f"{v['name']}-{g}-h{s:g}" for v, g, s in GEGLU_CASES])
def test_geglu_family_property_and_reference_error(v, gates, hscale):
    c = A.geglu_case(v, gates, hscale)
    ok, what = A.check_property("gate", gates, c.p[:, v["inner"]:])
    assert ok, f"{c.what}: {what}"
    assert v["rows"] % 2 == 1 or v["name"] == "geglu-second-trip"
    found = A.input_conditions(c)
    print(f"{c.what}: {what}; fp32 reference " + ", ".join(f"{k} {e:.1e}" for k, e in found.items()))


def test_tails_are_where_one_plus_erf_cancels():
    """What the `tails` family is for: at g = -3 .. -6, 1 + erf(g / sqrt 2) is 1e-3 .. 1e-9, so its fp32 value keeps few digits."""
    g = -A.make_gates("tails", 64, 64, 5).abs().double()
    s = 1 + torch.erf(g / 2 ** 0.5)
    assert s.max().item() < 3e-3 and s.min().item() < 1e-7


@pytest.mark.parametrize("v", A.GN_VARIANTS + A.LN_VARIANTS, ids=[v["name"] for v in A.GN_VARIANTS + A.LN_VARIANTS])
def test_variant_shape_reaches_its_launch_plan(v, lib):
    print(v["name"], A.assert_plan(lib, v))


def test_every_listed_form_is_reached():
    gn = A.GN_VARIANTS

    def has(kind, **want):
        return any(v["kind"] == kind and all(v["reach"].get(k) == x for k, x in want.items()) for v in gn)
    for vpt in A.GN_FWD_VPT:                                       # each one-pass size: a row that fills it, and (past the first) the
        fills = [v for v in gn if v["kind"] == "fwd_bwd" and v["L"] == 4096 * vpt]         # first row that needs it
        assert fills and fills[0]["reach"]["fwd"] == vpt
    for prev, vpt in zip(A.GN_FWD_VPT, A.GN_FWD_VPT[1:]):
        assert any(v["L"] == 4096 * prev + 4 and v["reach"]["fwd"] == vpt for v in gn)
    for vpt in A.GN_BWD_VPT:
        assert any(v["L"] == 4096 * vpt and v["reach"].get("bwd") == vpt for v in gn)
    for prev, vpt in zip(A.GN_BWD_VPT, A.GN_BWD_VPT[1:]):
        assert any(v["L"] == 4096 * prev + 4 and v["reach"].get("bwd") == vpt for v in gn)
    assert any(v["L"] == 36 for v in gn) and has("fwd_bwd", fwd=16, bwd=0)
    for nsplit in (8, 16, 64):
        assert has("fwd_bwd", fwd=0, bwd=0, nsplit=nsplit)
    for v in gn:
        if v["reach"].get("fwd") == 0 and "nsplit" in v["reach"]:   # no nsplit divides the row, the last split is ragged
            lo, hi = A.gn_splits(v["L"], v["reach"]["nsplit"])[-1]
            assert (v["L"] // 4) % v["reach"]["nsplit"] and (hi - lo) % 256 and hi > lo
    assert has("fork", fwd=2, bwd=2) and has("fork", fwd=0, bwd=0) and has("blocks", fwd=0)
    coef = [v for v in gn if v["kind"] == "coef"]
    assert {v["nblk"] for v in coef if v["L"] < 4096} == {0, 1, 3, 64} and {v["nblk"] for v in coef if v["L"] > 65536} == {0, 64}
    per_group = {(v["shape"][1] // v["shape"][2]) * v["nblk"] for v in gn if v["nblk"]}
    assert min(per_group) < 256 < max(per_group)
    assert any(v["shape"][2] == 1 for v in gn) and any(v["shape"][1] == v["shape"][2] for v in gn)
    assert any(v["shape"][1] == 96 and v["shape"][1] // v["shape"][2] == 3 for v in gn)
    forms = {}
    for v in gn:                                                   # every form meets every family, every eps, off, SiLU on and off
        for f in set(A.gn_forms(v).values()):
            d = forms.setdefault(f, {"families": set(), "eps": set(), "off": set(), "silu": set(), "dy": set()})
            d["families"] |= set(v["families"]); d["eps"].add(v["eps"]); d["off"].add(v["off"]); d["silu"].add(v["silu"])
            if f.endswith("bwd"):
                d["dy"] |= {A.dy_family(v, fam) for fam in v["families"]}
    assert set(forms) == {k for k in A.M if k.startswith("gn_")}
    for f, d in forms.items():
        assert d["families"] == set(A.GN_FAMILIES) and d["eps"] == {1e-5, 1e-6} and d["off"] == {True, False}, (f, d)
        assert d["silu"] == ({False} if f == "gn_coef" else {True, False}), (f, d)
        assert not f.endswith("bwd") or d["dy"] == set(A.DY_FAMILIES), (f, d)
    reach = A.ln_reachable()                                       # LayerNorm: every (lanes, float4) the plan can return
    assert 6 < len(reach) <= 28
    assert {v["reach"] for v in A.LN_VARIANTS} == set(reach)
    for C in (320, 640, 768, 1024, 1280):
        rpb = A.ln_rows_per_block(A.ln_plan(C)[0])
        assert {v["rows"] for v in A.LN_VARIANTS if v["C"] == C} >= {1, rpb - 1, rpb + 1, 4097}
    for key in ("with_d", "dskip"):
        assert {v[key] for v in A.LN_VARIANTS} == {True, False}
    assert {f for v in A.LN_VARIANTS for f in v["families"]} == set(A.LN_FAMILIES)
    assert {v["inner"] for v in A.GEGLU_VARIANTS} == {4, 1280, 5120}
    assert any(v["rows"] * v["inner"] // 4 > 16384 * 256 for v in A.GEGLU_VARIANTS)
    assert any(n * c * h * w // 4 > 8192 * 256 * 4 for n, c, h, w in A.BIAS_RESIDUAL_SHAPES)
    assert any(h * w == 4 for _, _, h, w in A.BIAS_RESIDUAL_SHAPES) and any(c == 1 for _, c, _, _ in A.BIAS_RESIDUAL_SHAPES)


def test_restated_plans_against_the_library_over_a_sweep(lib):
    for C in range(0, 2100, 4):
        assert lib.skp_add_layer_norm_ok(C) == int(A.ln_plan(C) is not None), C
    for C in (2, 6, 321, -4):
        assert lib.skp_add_layer_norm_ok(C) == 0
    for N, C, G, HW in ((1, 32, 32, 4096), (1, 32, 32, 4100), (2, 320, 32, 1024), (8, 128, 32, 512 * 512), (2, 512, 32, 64 * 64),
                        (1, 4, 4, 65536), (1, 4, 4, 65540), (64, 32, 32, 65540), (3, 96, 32, 12), (1, 64, 1, 16384)):
        L = (C // G) * HW
        assert lib.skp_group_norm_onepass_ok(N, C, G, HW) == int(A.gn_onepass_vpt(L, False) > 0), (N, C, G, HW)
        assert lib.skp_group_norm_nsplit(N, C, G, HW) == A.gn_nsplit(N, G, L), (N, C, G, HW)


def test_supported_and_refused_edges(lib):
    """N * G = 65 535 is the last grid the launchers accept; the width LayerNorm refuses is refused by plan and library alike."""
    from stablekeypoints_amd import ops

    def fake(N, C, H, W):                                          # group_norm_supported reads these four things of a tensor
        return types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 4, shape=(N, C, H, W))
    assert ops.group_norm_supported(fake(65535, 1, 2, 2), 1) and not ops.group_norm_supported(fake(65536, 1, 2, 2), 1)
    assert ops.group_norm_supported(fake(2047, 64, 2, 2), 32) and not ops.group_norm_supported(fake(2048, 64, 2, 2), 32)
    assert lib.skp_group_norm_nsplit(65535, 1, 1, 4) == 1 and lib.skp_group_norm_nsplit(65536, 1, 1, 4) == -2
    assert lib.skp_group_norm_nsplit(1, 6, 4, 4) == -2 and lib.skp_group_norm_nsplit(1, 4, 4, 6) == -2
    assert not ops.group_norm_supported(fake(1, 6, 2, 2), 4) and not ops.group_norm_supported(fake(1, 4, 1, 6), 4)
    assert A.ln_plan(A.LN_REFUSED_WIDTH) is None and lib.skp_add_layer_norm_ok(A.LN_REFUSED_WIDTH) == 0


def test_metric_and_bound():
    """The metric judges a huge element relatively and the bulk against the row's rms; the bound rejects a subtly wrong row."""
    y64 = torch.ones(2, 100, dtype=torch.float64)
    y64[0, 0] = 1000.0
    y = y64.clone().float()
    y[0, 0] += 1.0                                                 # 1e-3 of the huge element
    assert abs(A.row_err(y, y64, 2) - 1.0 / (1000 + (1e6 / 100 + 0.99) ** 0.5)) < 1e-6
    y = y64.clone().float()
    y[1, 5] += 1e-5                                                # 1e-5 / (1 + 1) in the row without the outlier
    assert abs(A.row_err(y, y64, 2) - 0.5e-5) < 1e-7
    assert A.bound(0.0, 4) == 4 * 2.0 ** -23 + 1e-7 and A.bound(1e-5, 4) == 4e-5 + 1e-7
    y[1, 5] = float("nan")
    assert A.row_err(y, y64, 2) != A.row_err(y, y64, 2)            # NaN: every comparison with it fails
    zero = torch.zeros(1, 8, dtype=torch.float64)
    assert A.row_err(zero.float(), zero, 1) == 0.0 and A.row_err(zero.float() + 1e-30, zero, 1) > 1e6
    c = A.gn_case(A.GN_BY_NAME["onepass-first-2"], "first_outlier")
    wrong = c.ref64["rstd"].float() * (1 + 1.5e-4)                 # what a shift by the outlier did to rstd at 65 536 elements
    with pytest.raises(AssertionError):
        A.assert_close({"rstd": wrong}, c, "gn_onepass_fwd")
    A.assert_close({k: t.clone() for k, t in c.ref32.items()}, c, A.gn_forms(c.v))
    assert all(m <= 8 for m in A.M.values())
