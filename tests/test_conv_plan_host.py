"""CPU tests of `ops.conv3x3_plan` / `ops.ConvPlan`, the one decision behind every stride-1 3x3 convolution route.

The decision table: over `_conv_cases.PLAN_GRID` (shapes x mode x own-kernels x GN_ONEPASS x direction x want_stats x
wino_raw_max_tiles, and a few rows with `_rows_per_launch` patched or the K split forced) the plan answers what the separate predicates and
`_conv3x3_run` of the commit before it answered; those answers are tests/golden/conv_plan_table.json (recorded with the dozen
lines in profiles/conv_plan.md).  One deliberate difference, stated where it is applied below: the fold verdict now needs a
`conv3x3_supported` shape.  The refusals: what a plan does not serve raises, naming the caller, before `_launch` is reached."""
import contextlib
import json
import os

import pytest
import torch

import _conv_cases as A
from stablekeypoints_amd import _native as N
from stablekeypoints_amd import ops

TABLE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "conv_plan_table.json")))
ROWS = [dict(zip(TABLE["columns"], r)) for r in TABLE["rows"]]


@contextlib.contextmanager
def switches(g):
    """The module switches and library overrides of grid entry `g`, restored on exit."""
    keep = ops.CONV3X3_MODE, ops.GN_ONEPASS, ops._rows_per_launch
    ops.CONV3X3_MODE, ops.GN_ONEPASS = g["mode"], g["onepass"]
    if g["rows_cap"]:
        ops._rows_per_launch = lambda *a: g["rows_cap"]
    N.tune("wino_raw_max_tiles", g["raw_tiles"])
    N.tune("wino_split", g["wino_split"])
    try:
        with (ops.conv3x3_own_kernels() if g["own"] else contextlib.nullcontext()):
            yield
    finally:
        ops.CONV3X3_MODE, ops.GN_ONEPASS, ops._rows_per_launch = keep
        N.tune("wino_raw_max_tiles", 0)
        N.tune("wino_split", 0)


def _shapes(g):
    B, ci, co, H, W = g["shape"]
    return (B, ci, H, W), (co, ci, 3, 3)


def test_table_matches_the_grid():
    assert tuple(TABLE["columns"]) == A.PLAN_COLUMNS and len(ROWS) == len(A.PLAN_GRID)
    assert {s for s, _ in A.PLAN_SHAPES} == {g["shape"] for g in A.PLAN_GRID if not (g["rows_cap"] or g["wino_split"])}


def test_plan_reproduces_the_recorded_decisions():
    bad = []

    def same(g, what, got, want):
        if got != want:
            bad.append(f"{g}: {what} is {got!r}, recorded {want!r}")
    for g, r in zip(A.PLAN_GRID, ROWS):
        xs, ws = _shapes(g)
        with switches(g):
            plan = ops.conv3x3_plan(xs, ws, backward=g["backward"], want_stats=g["want_stats"])
            same(g, "conv3x3_supported", bool(ops.conv3x3_supported(xs, ws)), r["supported"])
            same(g, "conv3x3_wanted", bool(ops.conv3x3_wanted(xs, ws)), r["wanted"])
            same(g, "conv3x3_f4_ok", bool(ops.conv3x3_f4_ok(xs, ws)), r["f4"])
            same(g, "conv3x3_f4r_ok", bool(ops.conv3x3_f4r_ok(xs, ws[0])), r["f4r"])
            same(g, "plan", tuple(plan), ("conv3x3.bwd_data" if g["backward"] else "conv3x3", r["kernel_route"] if r["wanted"] else "lib",
                                          r["form"], r["rows"], r["nblk"], 256, False))
            if r["nblk"] == 0:                            # ops.conv3x3: the kernels on every supported shape, whatever the tile rules say
                forced = ops.conv3x3_plan(xs, ws, backward=g["backward"], forced=True)
                same(g, "forced route", forced.route, r["kernel_route"] if r["supported"] else "lib")
            if g["want_stats"] and not g["onepass"] and not g["backward"] and r["wanted"]:
                same(g, "conv3x3_stats_blocks", ops.conv3x3_stats_blocks(xs, ws), r["nblk"])
            if not g["backward"]:
                # `supported and`: the earlier conv3x3_gn_fold_ok did not ask conv3x3_supported, so the 2^31-byte image of the grid passed
                # it and was refused by the launch (SKP_E_RANGE); the plan's first rule now holds for the fold as well
                fold = r["supported"] and r["fold_shape"] and r["gn_full"] and r["gn_tail"] is not False
                folded = ops.conv3x3_plan(xs, ws, want_stats=g["want_stats"], gn_fold=A.GN_GROUPS)
                want = plan._replace(fold=True, route="wino4_c128", form="f4") if fold else plan    # (the route conv3x3_gn_silu noted)
                if plan.form == "f4r" and xs[0] * (xs[2] // 4) * (xs[3] // 4) >= 32:     # a fold request does not ask for the raw form
                    want = plan._replace(form="f4", route=ops.routes.wino4_form(ws[0], r["rows"], xs[2], xs[3]))
                same(g, "fold plan", tuple(folded), tuple(want))
    assert not bad, f"{len(bad)} differences, the first: " + " | ".join(bad[:5])


def test_table_covers_every_decision():
    lib = N.lib()
    routes = {r["kernel_route"] if r["wanted"] else "lib" for r in ROWS}
    assert routes == {"wino4_raw", "wino4_c128", "wino4_c64", "wino2", "lib"}
    for col in ("supported", "wanted", "f4", "f4r", "fold_shape", "gn_full"):
        assert {r[col] for r in ROWS} == {True, False}, col
    assert {r["gn_tail"] for r in ROWS} == {True, False, None}
    assert {r["form"] for r in ROWS} == {"f4", "f4r", "f2"}
    assert any(r["rows"] < g["shape"][0] for g, r in zip(A.PLAN_GRID, ROWS))
    assert any(r["nblk"] > 0 for r in ROWS)
    chunked = [g["shape"] for g, r in zip(A.PLAN_GRID, ROWS)      # no statistics BECAUSE of the chunks: every other condition holds
               if g["want_stats"] and not g["onepass"] and not g["backward"] and r["wanted"] and r["f4"] and r["nblk"] == 0
               and r["rows"] < g["shape"][0] and lib.skp_conv3x3_f4_stats_blocks(*g["shape"]) > 0]
    assert chunked


class CountingLib:
    """The library with every host query (`*_ok`, `*_stats_blocks`) counted per (name, arguments)."""

    def __init__(self, lib):
        self.lib, self.asked = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not (name.endswith("_ok") or name.endswith("_stats_blocks")):
            return fn

        def counted(*args):
            self.asked[(name, args)] = self.asked.get((name, args), 0) + 1
            return fn(*args)
        return counted


def test_plan_asks_each_query_at_most_once_and_only_where_it_matters(monkeypatch):
    lib = CountingLib(N.lib())
    monkeypatch.setattr(ops.N, "lib", lambda: lib)
    for g in A.PLAN_GRID:
        xs, ws = _shapes(g)
        with switches(g):
            for kw in (dict(), dict(gn_fold=A.GN_GROUPS)):
                lib.asked.clear()
                plan = ops.conv3x3_plan(xs, ws, backward=g["backward"], want_stats=g["want_stats"], **kw)
                names = [n for n, _ in lib.asked]
                assert all(c == 1 for c in lib.asked.values()), (g, lib.asked)
                assert names.count("skp_conv3x3_f4_gn_ok") <= 2 and all(names.count(n) == 1 for n in names if n != "skp_conv3x3_f4_gn_ok")
                if g["mode"] != "f4" or xs[2] % 4 or xs[3] % 4 or ws[0] % 16 or ws[1] % 16:
                    assert not names, (g, names)          # F(4x4) out of the question: nothing to ask the library
                if g["backward"] or not g["want_stats"]:
                    assert not {"skp_conv3x3_f4_stats_blocks", "skp_group_norm_onepass_ok"} & set(names), (g, names)
                if plan.nblk or kw or plan.route == "lib":         # the raw form is asked about only where it decides something
                    assert "skp_conv3x3_f4r_ok" not in names or xs[0] * (xs[2] // 4) * (xs[3] // 4) < 32, (g, kw, names)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: shapes only (meta tensors), `_dev` let through, and any launch or filter build fails the test
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def fail(*a, **k):
        pytest.fail("a kernel was launched for a request the plan does not serve")
    monkeypatch.setattr(ops, "_launch", fail)
    monkeypatch.setattr(ops, "_filters", fail)
    monkeypatch.setattr(ops, "_dev", lambda t, name: t)
    monkeypatch.setattr(ops, "GN_ONEPASS", False)
    ops.routes.reset()
    yield
    assert ops.routes.snapshot() == {}, "a route was noted for a launch that was refused"


def _meta(*shape):
    return torch.empty(*shape, device="meta")


F4 = (2, 32, 128, 32, 32)          # F(4x4), 4 statistics blocks per image, served by the folded kernel
F2 = (8, 320, 320, 66, 64)         # H % 4 != 0: F(2x2)


def _operands(shape):
    B, ci, co, H, W = shape
    return _meta(B, ci, H, W), _meta(co, ci, 3, 3)


def test_statistics_on_a_plan_that_is_not_f4_are_refused(no_launch):
    x, w = _operands(F2)
    plan = ops.conv3x3_plan(x.shape, w.shape, want_stats=True)
    assert plan.form == "f2" and plan.nblk == 0
    with pytest.raises(RuntimeError, match=r"^conv3x3: block statistics on a plan of form f2"):
        ops.Conv3x3Fn.apply(x, w, None, None, _meta(8, 320, 16, 2), plan)


def test_statistics_of_another_block_count_are_refused(no_launch):
    x, w = _operands(F4)
    plan = ops.conv3x3_plan(x.shape, w.shape, want_stats=True)
    assert plan.form == "f4" and plan.nblk == 4
    with pytest.raises(RuntimeError, match=r"^conv3x3: statistics of shape \(2, 128, 8, 2\), the plan leaves \(2, 128, 4, 2\)"):
        ops.Conv3x3Fn.apply(x, w, None, None, _meta(2, 128, 8, 2), plan)


@pytest.mark.parametrize("entry", ["conv3x3", "conv3x3_gn_silu"])
def test_a_residual_of_another_shape_is_refused(no_launch, entry):
    x, w = _operands(F4)
    res = _meta(2, 128, 32, 16)
    with pytest.raises(RuntimeError, match=rf"^{entry}: residual of shape \(2, 128, 32, 16\), the output has \(2, 128, 32, 32\)"):
        if entry == "conv3x3":
            ops.conv3x3(x, w, None, res)
        else:
            ops.conv3x3_gn_silu(x, torch.nn.GroupNorm(32, 32), w, residual=res)


def test_a_fold_the_kernel_does_not_serve_is_refused(no_launch):
    x, w = _operands((1,) + F4[1:])                        # one row: 64 tiles, the 64-channel form
    assert not ops.conv3x3_plan(x.shape, w.shape, gn_fold=32).fold
    with pytest.raises(RuntimeError, match=r"^conv3x3_gn_silu: the folded kernel does not serve this launch"):
        ops.conv3x3_gn_silu(x, torch.nn.GroupNorm(32, 32), w)


def test_a_plan_without_a_kernel_is_refused(no_launch):
    x, w = _operands((1, 32, 32, 4, 4))
    plan = ops.conv3x3_plan(x.shape, w.shape)
    assert plan.route == "lib"
    with pytest.raises(RuntimeError, match=r"^conv3x3: the Winograd kernels are not planned for x \(1, 32, 4, 4\)"):
        ops.Conv3x3Fn.apply(x, w, None, None, None, plan)
    with pytest.raises(ValueError, match="unsupported shape"):    # (ops.conv3x3 keeps its own error for a shape no kernel takes)
        ops.conv3x3(*_operands((1, 16, 80, 12, 12)))
