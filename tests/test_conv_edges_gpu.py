"""The 3x3 convolution kernels against fp64 on hard activations (tests/_conv_cases.py): Winograd F(4x4,3x3) with transformed and
with raw filters, its statistics epilogue and its GroupNorm-folded form, Winograd F(2x2,3x3), the direct stride-2 kernel, the
small-input kernel, and the three that came with image sampling: the polyphase Winograd F(4x4,2x2) stride-2 kernel with its
statistics epilogue (`s2w`), nearest 2x up-sampling + convolution (`up2`) and the small-output kernel with its image epilogue
(`out`; as the input gradient of `ops.ConvInFn`: `in_fn`) -- every launch plan of each, on every input family.

Per case (kernel variant x family):
  * y (and dx where the variant has a backward-data launch) within  M[kernel family] x the per-plane error of the fp32 CPU
    reference that runs the same algorithm  (+1e-7) of fp64, everything finite;
  * a second call gives the same bits; where the variant has a routed entry (ops.conv3x3, conv3x3_gn_silu, conv3x3_s2,
    conv3x3_small, conv3x3_up2, conv3x3_small_out, ConvInFn) the first call goes through it, the second through the raw entry
    points: same bits again, and the route ledger shows the expected (site, route) once;
  * `out`: the launch with the image epilogue gives clamp(y / 2 + 0.5, 0, 1) of the plain launch's y, bit for bit, within the
    bound derived from y's (A.assert_image_close);
  * the launch plan the shape was chosen for is the one the library plans (its host queries) and the restated grid describes.
Per variant, on dc: every tensor inside NaN guard bands, output and workspace pre-filled with NaN, the workspace exactly the
queried size: same bits, finite, guards untouched.

Run with -s for one line per output: `conv-edge <variant> <family> <output>: err, fp32ref, ratio` (profiles/conv_edges.md)."""
import math
import time

import pytest
import torch

import _conv_cases as A

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of guard band on each side (256 bytes: the interior keeps its 16-byte alignment)
GUARD_BITS = 0x7FC0BEEF         # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Arena:
    """Device tensors of one launch, outputs pre-filled with NaN; `guarded`: each in the interior of its own larger buffer
    with GUARD floats of a marked NaN on both sides."""

    def __init__(self, guarded):
        self.guarded, self.bufs = guarded, []

    def empty(self, *shape):
        n = math.prod(shape)
        if not self.guarded:
            return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)
        buf = torch.empty(n + 2 * GUARD, device="cuda", dtype=torch.float32)
        buf.view(torch.int32).fill_(GUARD_BITS)
        self.bufs.append((buf, n))
        t = buf[GUARD:GUARD + n].view(shape)
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        return t

    def put(self, t):
        return None if t is None else self.empty(*t.shape).copy_(t)

    def workspace(self, nbytes):
        assert nbytes >= 0 and nbytes % 4 == 0
        return self.empty(nbytes // 4) if nbytes else None

    def intact(self):
        return all(bool((b.view(torch.int32)[:GUARD] == GUARD_BITS).all()) and bool((b.view(torch.int32)[GUARD + n:] == GUARD_BITS).all())
                   for b, n in self.bufs)


def guarded_hip(fn):
    """An error of the HIP runtime (a failed launch, a fault reported at the synchronisation) ends the session: nothing more may
    start on that device."""
    def run(ops, v, c, *args, **kw):
        try:
            return fn(ops, v, c, *args, **kw)
        except RuntimeError as e:
            if "hip" in str(e).lower():
                pytest.exit(f"{v['name']} on {c.family}: {e}", returncode=3)
            raise
    return run


def _filter(ops, arena, w, entry, per_pair, *dims):
    U = arena.empty(per_pair * w.shape[0] * w.shape[1])
    ops.N.check(getattr(ops.N.lib(), entry)(w.data_ptr(), U.data_ptr(), *dims, ops._stream()), entry)
    return U


@guarded_hip
def run_raw(ops, v, c, arena):
    """Variant `v` on case `c` through the raw entry points, every tensor from `arena` -> name -> device tensor."""
    lib, st, kind = ops.N.lib(), ops._stream(), v["kind"]
    B, ci, co, H, W = v["shape"]
    x, w, bias, res = arena.put(c.x), arena.put(c.w), arena.put(c.bias), arena.put(c.res)
    out = {}
    if kind in ("f4", "f4_stats"):
        U = _filter(ops, arena, w, "skp_conv3x3_f4_filter_f32", 36, co, ci, 0)
        out["y"] = ops._conv3x3_f4_raw(x, U, bias, co, split=v["split"], residual=res, out=arena.empty(B, co, H, W))
        if kind == "f4_stats":
            nblk = lib.skp_conv3x3_f4_stats_blocks(B, ci, co, H, W)
            out["stats"] = arena.empty(B, co, nblk, 2)
            out["y_stats"] = ops._conv3x3_f4_raw(x, U, bias, co, residual=res, out=arena.empty(B, co, H, W), stats=out["stats"])
    elif kind == "gn":
        G = A.GN_GROUPS
        gamma, beta, off = arena.put(c.gamma), arena.put(c.beta), arena.put(c.off)
        mean, rstd, coef, ws = arena.empty(B, G), arena.empty(B, G), arena.empty(B, ci, 2), arena.empty(B * G * 64 * 3)
        ops.N.check(lib.skp_group_norm_coef_f32(x.data_ptr(), ops._ptr(off), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), coef.data_ptr(), None, 0, 0, ws.data_ptr(), B, ci, G, H * W,
                                                float(A.GN_EPS), st), "skp_group_norm_coef_f32")
        U = _filter(ops, arena, w, "skp_conv3x3_f4_filter_f32", 36, co, ci, 0)
        out["y"] = arena.empty(B, co, H, W)
        if v["stats"]:
            out["stats"] = arena.empty(B, co, lib.skp_conv3x3_f4_stats_blocks(B, ci, co, H, W), 2)
        ops.N.check(lib.skp_conv3x3_f4_gn_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), ops._ptr(res), out["y"].data_ptr(),
                                              ops._ptr(out.get("stats")), coef.data_ptr(), B, ci, co, H, W, st), "skp_conv3x3_f4_gn_f32")
    elif kind == "f4r":
        R = _filter(ops, arena, w, "skp_conv3x3_f4r_filter_f32", 9, co, ci, 0)
        out["y"] = ops._conv3x3_f4r_raw(x, R, bias, co, residual=res, out=arena.empty(B, co, H, W))
    elif kind == "f2":
        U = _filter(ops, arena, w, "skp_conv3x3_filter_f32", 16, co, ci, 0)
        out["y"] = ops._conv3x3_raw(x, U, bias, co, variant=v["variant"], split=v["split"], residual=res, out=arena.empty(B, co, H, W))
    elif kind in ("s2", "s2_fn"):
        U = _filter(ops, arena, w, "skp_conv3x3_s2_filter_f32", 9, co, ci)
        out["y"] = arena.empty(B, co, H // 2, W // 2)
        if v["ws"] or kind == "s2_fn":                    # (ops._conv3x3_s2_raw always asks; 0 bytes = a null pointer)
            ws = ops._workspace("skp_conv3x3_s2_workspace", B, ci, co, H, W, device=x.device)
            ops.N.check(lib.skp_conv3x3_s2_ws_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), out["y"].data_ptr(), ops._ptr(ws),
                                                  B, ci, co, H, W, v["pad"], st), "skp_conv3x3_s2_ws_f32")
        else:
            ops.N.check(lib.skp_conv3x3_s2_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), out["y"].data_ptr(), B, ci, co, H, W,
                                               v["pad"], st), "skp_conv3x3_s2_f32")
    elif kind == "s2w":
        U = _filter(ops, arena, w, "skp_conv3x3_s2w_filter_f32", 81, co, ci, 0)
        out["y"] = arena.empty(B, co, H // 2, W // 2)
        ops.N.check(lib.skp_conv3x3_s2w_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), out["y"].data_ptr(), B, ci, co, H, W, 0, st),
                    "skp_conv3x3_s2w_f32")
        if v["stats"]:
            out["stats"], out["y_stats"] = arena.empty(B, co, (H // 8) * (W // 8) // 16, 2), arena.empty(B, co, H // 2, W // 2)
            ops.N.check(lib.skp_conv3x3_s2w_stats_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), out["y_stats"].data_ptr(),
                                                      out["stats"].data_ptr(), B, ci, co, H, W, 0, st), "skp_conv3x3_s2w_stats_f32")
    elif kind == "up2":
        U = _filter(ops, arena, w, "skp_conv3x3_up2_filter_f32", 16, co, ci)
        out["y"] = arena.empty(B, co, 2 * H, 2 * W)
        ops.N.check(lib.skp_conv3x3_up2_f32(x.data_ptr(), U.data_ptr(), ops._ptr(bias), out["y"].data_ptr(), B, ci, co, H, W, st),
                    "skp_conv3x3_up2_f32")
    elif kind == "out":
        for name, image in (("y", 0), ("img", 1)):
            out[name] = arena.empty(B, co, H, W)
            ops.N.check(lib.skp_conv3x3_small_out_f32(x.data_ptr(), w.data_ptr(), ops._ptr(bias), out[name].data_ptr(), B, ci, co, H, W,
                                                      image, st), "skp_conv3x3_small_out_f32")
    else:
        out["y"] = arena.empty(B, co, H, W)
        ops.N.check(lib.skp_conv3x3_small_f32(x.data_ptr(), w.data_ptr(), ops._ptr(bias), out["y"].data_ptr(), B, ci, co, H, W, st),
                    "skp_conv3x3_small_f32")
    if kind == "in_fn":                                   # the small-output kernel on dy with the rotated, transposed filter
        dy, wt = arena.put(c.dy), arena.put(A.backward_filter(c.w))
        out["dx"] = arena.empty(B, ci, H, W)
        ops.N.check(lib.skp_conv3x3_small_out_f32(dy.data_ptr(), wt.data_ptr(), None, out["dx"].data_ptr(), B, co, ci, H, W, 0, st),
                    "skp_conv3x3_small_out_f32")
    elif v["bwd"]:                                        # the same kernel on dy with the rotated, transposed filter
        dy = arena.put(c.dy if kind != "s2_fn" else A.zero_stuffed(c.dy, v["pad"], H, W))
        dx = arena.empty(B, ci, H, W)
        if kind in ("f4", "s2_fn"):
            Ub = _filter(ops, arena, w, "skp_conv3x3_f4_filter_f32", 36, ci, co, 1)
            out["dx"] = ops._conv3x3_f4_raw(dy, Ub, None, ci, split=v["split"], out=dx)
        elif kind == "f4r":
            Rb = _filter(ops, arena, w, "skp_conv3x3_f4r_filter_f32", 9, ci, co, 1)
            out["dx"] = ops._conv3x3_f4r_raw(dy, Rb, None, ci, out=dx)
        else:
            assert kind == "f2"
            Ub = _filter(ops, arena, w, "skp_conv3x3_filter_f32", 16, ci, co, 1)
            out["dx"] = ops._conv3x3_raw(dy, Ub, None, ci, variant=v["variant"], split=v["split"], out=dx)
    torch.cuda.synchronize()
    return out


@guarded_hip
def run_routed(ops, v, c):
    """Variant `v` through its routed entry -> name -> device tensor."""
    kind = v["kind"]
    x, w = c.x.cuda(), c.w.cuda()
    bias, res = (None if c.bias is None else c.bias.cuda()), (None if c.res is None else c.res.cuda())
    out = {}
    if v["bwd"]:
        x.requires_grad_(True)
    if kind == "f4":
        y = ops.conv3x3(x, w, bias, res)
    elif kind == "gn":
        norm = torch.nn.GroupNorm(A.GN_GROUPS, x.shape[1], eps=A.GN_EPS).cuda().requires_grad_(False)
        norm.weight.copy_(c.gamma)
        norm.bias.copy_(c.beta)
        y = ops.conv3x3_gn_silu(x, norm, w, off=None if c.off is None else c.off.cuda(), bias=bias, residual=res, want_stats=v["stats"])
        if v["stats"]:
            assert getattr(y, "_skp_blocks", None) is not None, "this launch must leave block statistics behind"
            out["stats"] = y._skp_blocks[0]
    elif kind == "s2_fn":
        y = ops.conv3x3_s2(x, w, bias, pad=v["pad"])
    elif kind == "s2w":
        y = ops.conv3x3_s2(x, w, bias, pad=0, want_stats=v["stats"])
        assert (getattr(y, "_skp_blocks", None) is not None) == v["stats"], "statistics exactly where the variant asks for them"
        if v["stats"]:
            out["stats"] = y._skp_blocks[0]
    elif kind == "up2":
        with torch.no_grad():
            y = ops.conv3x3_up2(x, w, bias)
    elif kind == "out":
        assert ops.conv3x3_small_out_ok(x, w)
        y, out["img"] = ops.conv3x3_small_out(x, w, bias), ops.conv3x3_small_out(x, w, bias, image=True)
    elif kind == "in_fn":
        assert ops.conv_in_grad_ok(x, w)
        y = ops.ConvInFn.apply(x, w, bias)
    else:
        assert kind == "small"
        y = ops.conv3x3_small(x, w, bias, want_stats=v["stats"])
        assert getattr(y, "_skp_blocks", None) is None      # (no shape of this table is large enough for that kernel's statistics)
    out["y"] = y.detach()
    if v["bwd"]:
        out["dx"], = torch.autograd.grad(y, x, c.dy.cuda())
    torch.cuda.synchronize()
    return out


def routed_ledger(ops, v):
    led = A.expected_ledger(v)
    B, ci, co, H, W = v["shape"]
    if v["kind"] == "f4" and v["bwd"]:
        led[("conv3x3.bwd_data", ops.routes.wino4_form(ci, B, H, W))] = 1
    return led


def check_statistics(v, out):
    """{mean, M2} per block of 16 tiles against the fp64 statistics of the kernel's OWN y (the tolerances of
    test_epilogue_statistics_survive_a_large_channel_mean)."""
    y = out.get("y_stats", out["y"]).cpu()
    want = A.block_statistics(y, 4, 4)
    got = out["stats"].cpu().double()
    assert got.shape == want.shape
    print(f"conv-edge-stats {v['name']}: mean max abs err {(got[..., 0] - want[..., 0]).abs().max().item():.2e}, "
          f"M2 max err / max M2 {((got[..., 1] - want[..., 1]).abs().max() / want[..., 1].max()).item():.2e}")
    torch.testing.assert_close(got, want, rtol=1e-3, atol=2e-3)


CASES = [(v, f) for v in A.VARIANTS for f in v["families"]]


@pytest.mark.parametrize("v,family", CASES, ids=[f"{v['name']}-{f}" for v, f in CASES])
def test_conv_kernel_vs_fp64(ops, ncu, tune, monkeypatch, v, family):
    for key, value in v["tune"].items():
        tune(key, value)
    facts = A.assert_plan(ops, v, ncu)
    t0 = time.perf_counter()
    c = A.case(v, family)
    if v["routed"] is not None:
        if v["stats"]:
            monkeypatch.setattr(ops, "GN_ONEPASS", False)     # the convolution keeps its block sums at this small shape
        ops.routes.reset()
        first = run_routed(ops, v, c)
        assert ops.routes.snapshot() == routed_ledger(ops, v), ops.routes.table()
    else:
        first = run_raw(ops, v, c, Arena(False))
    second = run_raw(ops, v, c, Arena(False))
    A.assert_conv_close({name: first[name].cpu() for name in c.ref64}, c, v["name"])
    for name in first:
        assert torch.isfinite(second[name]).all(), name
        assert torch.equal(first[name], second[name]), f"{v['name']} {family}: {name} differs between two calls"
    if "y_stats" in second:
        assert torch.equal(second["y_stats"], second["y"]), "the statistics epilogue changes y"
    if v["kind"] == "out":
        A.assert_image_close(first["y"].cpu(), first["img"].cpu(), c, v["name"])
    if "stats" in second:
        check_statistics(v, second)
    print(f"conv-edge-time {v['name']} {family}: {time.perf_counter() - t0:.2f} s  {facts}")


@pytest.mark.parametrize("v", A.VARIANTS, ids=[v["name"] for v in A.VARIANTS])
def test_conv_kernel_stays_inside_its_buffers(ops, ncu, tune, monkeypatch, v):
    """dc (nothing cancels: a stray read shows) with x, the filters, bias, residual, y, statistics and GroupNorm coefficients
    between NaN guard bands, outputs and workspace pre-filled with NaN, and the workspace exactly as large as its query says:
    bit-equal to the plain call, finite, every guard untouched.  A kernel that reads past a ragged tile block or channel group and
    counts on 0 * x to drop it, writes past one, or counts on a zeroed workspace for its padded tiles, fails here.  Every byte
    touched lies inside a torch allocation."""
    for key, value in v["tune"].items():
        tune(key, value)
    A.assert_plan(ops, v, ncu)
    c = A.case(v, "dc")
    plain = run_raw(ops, v, c, Arena(False))
    arena = Arena(True)
    lib = ops.N.lib()
    sizes = []

    def exact_workspace(query, *args, device):
        sizes.append((query, int(getattr(lib, query)(*args))))
        return arena.workspace(sizes[-1][1])
    monkeypatch.setattr(ops, "_workspace", exact_workspace)
    guarded = run_raw(ops, v, c, arena)
    if v["kind"] in ("f4", "f4r", "f2") and v["split"]:
        assert sizes and all(q.endswith("_workspace") for q, _ in sizes)
        assert (sizes[0][1] > 0) == (v["reach"]["S"] > 1 or v["kind"] == "f4r")
    for name in plain:
        assert torch.isfinite(guarded[name]).all(), name
        assert torch.equal(plain[name], guarded[name]), f"{v['name']}: {name} changes when its neighbourhood is NaN"
    assert arena.intact(), f"{v['name']}: a guard band was written"


def test_every_caller_makes_one_plan_and_runs_it(ops, monkeypatch):
    """At (2,32,128,32,32): `conv3x3_auto` with statistics, `conv3x3_auto` on an input that takes a gradient, and that call's
    backward each make exactly ONE `conv3x3_plan`; `conv3x3_gn_fold_ok` + `conv3x3_gn_silu` note the route their plan names; and
    every output is bit-equal to the raw launchers called with the same filter."""
    v, vg = A.BY_NAME["f4-c128-one-group"], A.BY_NAME["gn-c128-smallest"]
    B, ci, co, H, W = v["shape"]
    assert vg["shape"] == v["shape"]
    c, cg = A.case(v, "randn"), A.case(vg, "randn")
    monkeypatch.setattr(ops, "GN_ONEPASS", False)         # the convolution keeps its block sums at this small shape
    plans, make = [], ops.conv3x3_plan
    monkeypatch.setattr(ops, "conv3x3_plan", lambda *a, **k: plans.append(make(*a, **k)) or plans[-1])
    x, w, bias, res, dy = (t.cuda() for t in (c.x, c.w, c.bias, c.res, c.dy))
    try:
        y = ops.conv3x3_auto(x, w, bias, res, want_stats=True)
        assert len(plans) == 1 and plans[0][1:5] == ("wino4_c128", "f4", B, 4), plans
        stats = torch.empty(B, co, 4, 2, device="cuda")
        assert torch.equal(y, ops._conv3x3_f4_raw(x, ops._wino4_filters(w, False), bias, co, residual=res, stats=stats))
        assert y._skp_blocks[1:] == (4, 256) and torch.equal(y._skp_blocks[0], stats)
        plans.clear()
        xg = x.clone().requires_grad_(True)
        y2 = ops.conv3x3_auto(xg, w, bias, res)
        assert len(plans) == 1 and plans[0].site == "conv3x3" and plans[0].nblk == 0, plans
        assert torch.equal(y2, y) and not hasattr(y2, "_skp_blocks")
        plans.clear()
        dx, = torch.autograd.grad(y2, xg, dy)
        assert len(plans) == 1 and plans[0].site == "conv3x3.bwd_data" and plans[0].route == ops.routes.wino4_form(ci, B, H, W), plans
        assert torch.equal(dx, ops._conv3x3_f4_raw(dy, ops._wino4_filters(w, True), None, ci))
        plans.clear()
        norm = torch.nn.GroupNorm(A.GN_GROUPS, ci, eps=A.GN_EPS).cuda().requires_grad_(False)
        norm.weight.copy_(cg.gamma)
        norm.bias.copy_(cg.beta)
        xn, wn, bn = cg.x.cuda(), cg.w.cuda(), cg.bias.cuda()
        ops.routes.reset()
        assert ops.conv3x3_gn_fold_ok(xn, norm, wn, None, bn, None)
        z = ops.conv3x3_gn_silu(xn, norm, wn, bias=bn)
        assert len(plans) == 2 and plans[0] == plans[1] and plans[1].fold, plans
        assert ops.routes.snapshot() == {("conv3x3", plans[1].route): 1, ("group_norm", "gn_fold"): 1, ("group_norm.stats", "own_pass"): 1}
        assert torch.equal(z, run_raw(ops, vg, cg, Arena(False))["y"])
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit(f"one plan per call: {e}", returncode=3)
        raise
    A.assert_conv_close({"y": y.cpu(), "dx": dx.cpu()}, c, "planned conv3x3_auto")
    A.assert_conv_close({"y": z.cpu()}, cg, "planned conv3x3_gn_silu")


def test_batch_chunking_without_2gib(ops, monkeypatch):
    """The batch-chunk loops of ops._conv3x3_run and ops.conv3x3_gn_silu (taken above 2 GiB per tensor) at 5 rows in chunks of 2, 2
    and 1: bit-equal to the five one-image calls."""
    v = dict(A.BY_NAME["gn-c128-off-stats"], shape=(5, 32, 128, 48, 48), name="chunked", stats=False)
    B, ci, co, H, W = v["shape"]
    lib = ops.N.lib()
    for rows in (2, 1):                                   # one launch form for the chunks and for the single images
        assert lib.skp_conv3x3_f4_gn_ok(rows, ci, co, H, W) == 1 and lib.skp_conv3x3_f4_workspace(rows, ci, co, H, W) == 0
    c = A.Case(v, "post_silu")
    x, w, bias, res, off = (t.cuda() for t in (c.x, c.w, c.bias, c.res, c.off))
    norm = torch.nn.GroupNorm(A.GN_GROUPS, ci, eps=A.GN_EPS).cuda().requires_grad_(False)
    norm.weight.copy_(c.gamma)
    norm.bias.copy_(c.beta)
    monkeypatch.setattr(ops, "_rows_per_launch", lambda *a: 2)
    try:
        ops.routes.reset()
        y = ops.conv3x3(x, w, bias, res)
        assert ops.routes.snapshot() == {("conv3x3", "wino4_c128"): 1}, ops.routes.table()
        assert ops.conv3x3_gn_fold_ok(x, norm, w, off, bias, res)
        z = ops.conv3x3_gn_silu(x, norm, w, off=off, bias=bias, residual=res)
        monkeypatch.undo()
        for i in range(B):
            assert torch.equal(y[i:i + 1], ops.conv3x3(x[i:i + 1].contiguous(), w, bias, res[i:i + 1].contiguous())), f"conv3x3, image {i}"
            zi = ops.conv3x3_gn_silu(x[i:i + 1].contiguous(), norm, w, off=off[i:i + 1], bias=bias, residual=res[i:i + 1].contiguous())
            assert torch.equal(z[i:i + 1], zi), f"conv3x3_gn_silu, image {i}"
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit(f"batch chunking: {e}", returncode=3)
        raise
    A.assert_conv_close({"y": z.cpu()}, c, "chunked gn")
    plain = dict(v, kind="f4", name="chunked-plain", mfam={"y": "f4"})
    A.assert_conv_close({"y": y.cpu()}, A.Case(plain, "post_silu"), "chunked conv3x3")
