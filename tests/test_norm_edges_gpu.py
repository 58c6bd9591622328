"""The normalisation and pointwise kernels against fp64 on hard activations (tests/_norm_cases.py): GroupNorm(+offset)(+SiLU) forward
and backward in its one-pass and two-kernel forms, the fork backward, the block-statistics consumer and the coefficient form,
add+LayerNorm, GEGLU, bias+residual and the two layout transposes -- every launch plan of each, on every input family.

Per case (kernel variant x family):
  * every output, and the saved statistics read from the library call itself, within  M[form] x max(the error of the fp32 CPU
    reference that runs the same algorithm, 2^-23) + 1e-7  of fp64 under the per-row metric, everything finite;
  * a second call gives the same bits;
  * x = d + h of add+LayerNorm, bias+residual and the transposes are bit-equal to the fp32 expression they stand for.
Per form, once: one NaN, and separately one +inf, in a single row makes that row's outputs NaN and leaves every other row
bit-identical to the run without it (outputs and workspace pre-filled with NaN throughout).

Run with -s for one line per output: `norm-edge <variant> <family> <form> <output>: err, fp32ref, ratio` (profiles/norm_edges.md)."""
import pytest
import torch

import _norm_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def dev(t):
    return None if t is None else t.cuda().contiguous()


def nans(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def ptr(t):
    return None if t is None else t.data_ptr()


def check(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def hip_guard(fn):
    """An error of the HIP runtime (a failed launch, a fault reported at the synchronisation) ends the session: nothing more may
    start on that device."""
    def run(*args, **kw):
        try:
            return fn(*args, **kw)
        except RuntimeError as e:
            if "hip" in str(e).lower():
                pytest.exit(f"{fn.__name__}: {e}", returncode=3)
            raise
    run.__name__ = fn.__name__
    return run


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
@hip_guard
def gn_launch(lib, st, v, x, off, gamma, beta, dy=None, dadd=None, bs=None):
    """Variant `v` through the library's entry points on device tensors -> name -> device tensor (outputs and the workspace start
    as NaN)."""
    N, C, G, H, W = v["shape"]
    HW, eps, silu = H * W, float(v["eps"]), int(v["silu"])
    mean, rstd, ws = nans(N, G), nans(N, G), nans(N * G * 64 * 3)
    nblk = v["nblk"]
    out = {"mean": mean, "rstd": rstd}
    if v["kind"] == "coef":
        coef = nans(N, C, 2)
        check(lib.skp_group_norm_coef_f32(None if nblk else x.data_ptr(), ptr(off), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                          rstd.data_ptr(), coef.data_ptr(), ptr(bs), nblk, HW // nblk if nblk else 0,
                                          None if nblk else ws.data_ptr(), N, C, G, HW, eps, st), "skp_group_norm_coef_f32")
        out["scale"], out["shift"] = coef[..., 0], coef[..., 1]
        torch.cuda.synchronize()
        return out
    y = nans(N, C, H, W)
    if v["kind"] == "blocks":
        check(lib.skp_group_norm_fwd_blocks_f32(x.data_ptr(), ptr(off), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                rstd.data_ptr(), bs.data_ptr(), nblk, HW // nblk, N, C, G, HW, eps, silu, st),
              "skp_group_norm_fwd_blocks_f32")
    else:
        check(lib.skp_group_norm_fwd_f32(x.data_ptr(), ptr(off), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                         rstd.data_ptr(), ws.data_ptr(), N, C, G, HW, eps, silu, st), "skp_group_norm_fwd_f32")
    out["y"] = y
    if v["bwd"]:
        dx, ws2 = nans(N, C, H, W), nans(N * G * 64 * 3)
        if v["kind"] == "fork":
            check(lib.skp_group_norm_bwd_add_f32(x.data_ptr(), ptr(off), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                                 rstd.data_ptr(), dx.data_ptr(), dadd.data_ptr(), ws2.data_ptr(), N, C, G, HW, eps, silu,
                                                 st), "skp_group_norm_bwd_add_f32")
        else:
            check(lib.skp_group_norm_bwd_f32(x.data_ptr(), ptr(off), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), mean.data_ptr(),
                                             rstd.data_ptr(), dx.data_ptr(), ws2.data_ptr(), N, C, G, HW, eps, silu, st),
                  "skp_group_norm_bwd_f32")
        out["dx"] = dx
    torch.cuda.synchronize()
    return out


def gn_run(lib, st, v, c, x=None, bs=None):
    x = c.x if x is None else x
    bs = c.bs if bs is None else bs
    return gn_launch(lib, st, v, dev(x), dev(c.off), dev(c.gamma), dev(c.beta), dev(c.dy), dev(c.dadd), dev(bs))


GN_CASES = [(v, f) for v in A.GN_VARIANTS for f in v["families"]]


@pytest.mark.parametrize("v,family", GN_CASES, ids=[f"{v['name']}-{f}" for v, f in GN_CASES])
def test_group_norm_against_fp64(ops, v, family):
    lib, st = ops.N.lib(), ops._stream()
    A.assert_plan(lib, v)
    c = A.gn_case(v, family)
    first, second = gn_run(lib, st, v, c), gn_run(lib, st, v, c)
    for name in first:
        assert same_bits(first[name], second[name]), f"{c.what} {name}: a second call gives other bits"
    A.assert_close({k: t.cpu() for k, t in first.items()}, c, A.gn_forms(v))


# one variant per form: (variant, family whose case supplies the clean inputs)
NONFINITE_GN = ["onepass-first-2", "onepass-fills-16-bwd-two-kernel", "two-kernel-nsplit-16-plain", "fork-onepass", "fork-two-kernel",
                "blocks-fwd-nblk-3", "coef-small-own-pass", "coef-large-own-pass", "coef-small-nblk-3"]


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", NONFINITE_GN)
def test_group_norm_non_finite_input_stays_in_its_row(ops, name, poison):
    lib, st, v = ops.N.lib(), ops._stream(), A.GN_BY_NAME[name]
    c = A.gn_case(v, "randn")
    N, C, G, H, W = v["shape"]
    rows, bad = N * G, (N * G) // 2
    x = c.x.clone()
    A.gn_rows(x, G)[bad, v["L"] // 3] = poison
    clean = gn_run(lib, st, v, c)
    got = gn_run(lib, st, v, c, x=x, bs=A.block_stats(x, v["nblk"]) if v["nblk"] else None)
    others = [r for r in range(rows) if r != bad]
    for key, t in got.items():
        a, b = t.cpu(), clean[key].cpu()
        a, b = (a.reshape(rows, -1), b.reshape(rows, -1))
        assert same_bits(a[others], b[others]), f"{name} {key}: a non-finite value in row {bad} changed another row"
        if key != "mean":                                          # (the mean of a row with +inf is +inf)
            assert bool(torch.isnan(a[bad]).all()), f"{name} {key}: row {bad} is not all NaN"
        else:
            assert not bool(torch.isfinite(a[bad]).any())


# ---------------------------------------------------------------------------------------------------------------------
# add + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@hip_guard
def ln_launch(lib, st, v, d, h, gamma, beta, dn, dskip):
    rows, C = h.shape
    n, stat, dx = nans(rows, C), nans(rows, 2), nans(rows, C)
    x = nans(rows, C) if d is not None else h
    check(lib.skp_add_layer_norm_fwd_f32(ptr(d), h.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.data_ptr() if d is not None else None,
                                         n.data_ptr(), stat.data_ptr(), rows, C, float(v["eps"]), st), "skp_add_layer_norm_fwd_f32")
    check(lib.skp_add_layer_norm_bwd_f32(dn.data_ptr(), ptr(dskip), x.data_ptr(), stat.data_ptr(), gamma.data_ptr(), dx.data_ptr(), rows,
                                         C, st), "skp_add_layer_norm_bwd_f32")
    torch.cuda.synchronize()
    return {"x": x, "n": n, "ln_mean": stat[:, 0], "ln_rstd": stat[:, 1], "dx": dx}


def ln_run(lib, st, v, c, h=None):
    return ln_launch(lib, st, v, dev(c.d), dev(c.h if h is None else h), dev(c.gamma), dev(c.beta), dev(c.dn), dev(c.dskip))


LN_FORMS = {"n": "ln_fwd", "ln_mean": "ln_fwd", "ln_rstd": "ln_fwd", "dx": "ln_bwd"}
LN_CASES = [(v, f) for v in A.LN_VARIANTS for f in v["families"]]


@pytest.mark.parametrize("v,family", LN_CASES, ids=[f"{v['name']}-{f}" for v, f in LN_CASES])
def test_add_layer_norm_against_fp64(ops, v, family):
    lib, st = ops.N.lib(), ops._stream()
    A.assert_plan(lib, v)
    c = A.ln_case(v, family)
    first, second = ln_run(lib, st, v, c), ln_run(lib, st, v, c)
    for name in first:
        assert same_bits(first[name], second[name]), f"{c.what} {name}: a second call gives other bits"
    assert same_bits(first.pop("x").cpu(), c.x), f"{c.what}: x is not fp32 d + h bit for bit"
    A.assert_close({k: t.cpu() for k, t in first.items()}, c, LN_FORMS)


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ["ln-w320-rows-17", "ln-w1280-rows-5"])
def test_add_layer_norm_non_finite_input_stays_in_its_row(ops, name, poison):
    lib, st, v = ops.N.lib(), ops._stream(), A.LN_BY_NAME[name]
    c = A.ln_case(v, "randn")
    bad = v["rows"] // 2
    h = c.h.clone()
    h[bad, v["C"] // 3] = poison
    clean, got = ln_run(lib, st, v, c), ln_run(lib, st, v, c, h=h)
    others = [r for r in range(v["rows"]) if r != bad]
    for key in ("n", "dx", "ln_rstd", "ln_mean"):
        a, b = got[key].cpu().reshape(v["rows"], -1), clean[key].cpu().reshape(v["rows"], -1)
        assert same_bits(a[others], b[others]), f"{name} {key}: a non-finite value in row {bad} changed another row"
        if key in ("n", "dx"):
            assert bool(torch.isnan(a[bad]).all()), f"{name} {key}: row {bad} is not all NaN"


def test_add_layer_norm_refuses_the_width_it_has_no_kernel_for(ops):
    """1792 = 4 * 7 * 64: the library says so on the host, the entry points return SKP_E_RANGE and touch nothing, and
    ops.add_layer_norm_supported sends the caller to the ordinary LayerNorm."""
    lib, st, C = ops.N.lib(), ops._stream(), A.LN_REFUSED_WIDTH
    assert A.ln_plan(C) is None and lib.skp_add_layer_norm_ok(C) == 0
    h, gamma, beta = torch.randn(5, C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    n, stat, dx = nans(5, C), nans(5, 2), nans(5, C)
    assert lib.skp_add_layer_norm_fwd_f32(None, h.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, n.data_ptr(), stat.data_ptr(), 5, C,
                                          1e-5, st) == -2
    assert lib.skp_add_layer_norm_bwd_f32(h.data_ptr(), None, h.data_ptr(), stat.data_ptr(), gamma.data_ptr(), dx.data_ptr(), 5, C, st) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(n).all()) and bool(torch.isnan(stat).all()) and bool(torch.isnan(dx).all())
    norm = torch.nn.LayerNorm(C).cuda().requires_grad_(False)
    assert not ops.add_layer_norm_supported(h, norm)
    assert ops.add_layer_norm_supported(h[:, :1280].contiguous(), torch.nn.LayerNorm(1280).cuda().requires_grad_(False))


# ---------------------------------------------------------------------------------------------------------------------
# GEGLU, bias + residual, the layout transposes
# ---------------------------------------------------------------------------------------------------------------------
@hip_guard
def geglu_launch(lib, st, p, dy):
    rows, inner = dy.shape
    y, dp = nans(rows, inner), nans(rows, 2 * inner)
    check(lib.skp_geglu_fwd_f32(p.data_ptr(), y.data_ptr(), rows, inner, st), "skp_geglu_fwd_f32")
    check(lib.skp_geglu_bwd_f32(p.data_ptr(), dy.data_ptr(), dp.data_ptr(), rows, inner, st), "skp_geglu_bwd_f32")
    torch.cuda.synchronize()
    return {"y": y, "dh": dp[:, :inner].contiguous(), "dg": dp[:, inner:].contiguous()}


GEGLU_CASES = [(v, g, s) for v in A.GEGLU_VARIANTS for g, s in v["cases"]]
GEGLU_FORMS = {"y": "geglu_fwd", "dh": "geglu_bwd", "dg": "geglu_bwd"}


@pytest.mark.parametrize("v,gates,hscale", GEGLU_CASES, ids=[f"{v['name']}-{g}-h{s:g}" for v, g, s in GEGLU_CASES])
def test_geglu_against_fp64(ops, v, gates, hscale):
    lib, st = ops.N.lib(), ops._stream()
    c = A.geglu_case(v, gates, hscale)
    p, dy = dev(c.p), dev(c.dy)
    first, second = geglu_launch(lib, st, p, dy), geglu_launch(lib, st, p, dy)
    for name in first:
        assert same_bits(first[name], second[name]), f"{c.what} {name}: a second call gives other bits"
    A.assert_close({k: t.cpu() for k, t in first.items()}, c, GEGLU_FORMS)


@pytest.mark.parametrize("shape", A.BIAS_RESIDUAL_SHAPES, ids=["x".join(map(str, s)) for s in A.BIAS_RESIDUAL_SHAPES])
def test_add_bias_residual_is_the_fp32_sum_bit_for_bit(ops, shape):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(53)
    a, b = torch.randn(shape, generator=g), 100 * torch.randn(shape, generator=g)
    bias = torch.randn(C, generator=g)
    want = (a + b) + bias[None, :, None, None]
    da, db, dbias = dev(a), dev(b), dev(bias)
    outs = []
    for _ in range(2):
        out = nans(*shape)
        check(ops.N.lib().skp_add_bias_residual_f32(da.data_ptr(), db.data_ptr(), dbias.data_ptr(), out.data_ptr(), N, C, H * W,
                                                    ops._stream()), "skp_add_bias_residual_f32")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert same_bits(outs[0], want), f"{shape}: not (a + b) + bias in fp32"
    assert same_bits(outs[0], outs[1])


@pytest.mark.parametrize("shape", A.LAYOUT_SHAPES, ids=["x".join(map(str, s)) for s in A.LAYOUT_SHAPES])
def test_layout_transposes_are_exact(ops, shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(59)
    x, res = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = torch.randn(B, H * W, C, generator=g)
    tokens = x.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
    nchw = t.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    dx, dres, dt = dev(x).requires_grad_(True), dev(res).requires_grad_(True), dev(t).requires_grad_(True)
    y = ops.nchw_to_tokens(dx)                                     # forward, and its gradient: the way back without a residual
    assert same_bits(y.detach().cpu(), tokens)
    y.backward(dt.detach())
    assert same_bits(dx.grad.cpu(), nchw)
    z = ops.tokens_to_nchw_add(dt, dres)                           # the way back with the residual, and both its gradients
    assert same_bits(z.detach().cpu(), nchw + res)
    z.backward(dx.detach())
    assert same_bits(dt.grad.cpu(), tokens) and same_bits(dres.grad.cpu(), x)
    assert same_bits(ops._to_nchw_raw(dt.detach(), None, H, W).cpu(), nchw)
