"""The text encoder on the MI355X: the causal attention kernel against fp64 over every boundary it has (tests/_text_cases.py), the
towers' routes and accuracy, and a prompt as the unconditional input of image sampling.

Kernel cases: N in {1, 2, 15, 16, 17, 31, 32, 33, 64, 77, 128} x d in {32, 64} x (B, H) in {(1, 1), (2, 3)} x {dense operands,
column bands of a packed q | k | v buffer} x nine input families, through the C ABI so that `out` can sit between NaN guard bands
(the packed buffer too: with ld = 3*H*d the three bands cover every column of a row, so the guards are the floats in front of
and behind it).  A third layout, `padded`, goes beyond the issue's two: rows of ld = 3*H*d + 4 floats whose first four columns no
band covers and hold NaN, the bands starting at columns 4, 4 + C and 4 + 2C -- the stride arithmetic apart from the band layout.
Nothing is skipped or filtered.
"""
import pytest
import torch

import _attn_cases as A
import _text_cases as T

pytestmark = pytest.mark.gpu

GUARD = 1024            # floats of NaN on either side of a buffer


def _guarded(t):
    """A copy of the CPU tensor `t` on the GPU between two NaN guard bands -> (view of the copy, the whole flat buffer)."""
    flat = torch.full((t.numel() + 2 * GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    body = flat[GUARD:GUARD + t.numel()].view(t.shape)
    body.copy_(t)
    return body, flat


def _guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all())


PAD = 4                 # unread NaN columns in front of the bands of the `padded` layout


def _run_kernel(c, layout):
    from stablekeypoints_amd import _native as N
    B, _, H, Nn, _, d = c.shape
    C = H * d
    packed = layout != "dense"
    if packed:
        pad = PAD if layout == "padded" else 0
        rows = torch.cat([torch.full((B, Nn, pad), float("nan")), c.q, c.k, c.v], dim=-1)
        body, src = _guarded(rows)
        q, k, v, ld = body[..., pad:pad + C], body[..., pad + C:pad + 2 * C], body[..., pad + 2 * C:], pad + 3 * C
    else:
        (q, sq), (k, sk), (v, sv) = _guarded(c.q), _guarded(c.k), _guarded(c.v)
        src, ld = None, C
    out, oflat = _guarded(torch.full((B, Nn, C), float("nan")))
    assert N.lib().skp_text_attn_fwd_ok(B, H, Nn, d, ld) == 1
    N.check(N.lib().skp_text_attn_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Nn, d, ld,
                                          float(c.scale), torch.cuda.current_stream().cuda_stream), "skp_text_attn_fwd_f32")
    torch.cuda.synchronize()
    assert _guards_intact(oflat), "the kernel wrote outside out"
    if packed:
        assert _guards_intact(src) and torch.equal(body.cpu()[..., pad:], rows[..., pad:]), "the inputs were touched"
        assert bool(torch.isnan(body[..., :pad]).all())
    return out.cpu()


@pytest.mark.parametrize("layout", ["dense", "packed", "padded"])
@pytest.mark.parametrize("B,H", T.BATCH_HEADS)
@pytest.mark.parametrize("d", T.HEAD_DIMS)
@pytest.mark.parametrize("N", T.SIZES)
def test_causal_kernel_vs_fp64(N, d, B, H, layout):
    for family in T.FAMILIES:
        c = T.case(family, B, H, N, d)
        got = _run_kernel(c, layout)
        A.assert_attn_close({"out": got}, c, T.M, f"text-attn {layout} N={N} d={d} B={B} H={H}")


def test_ops_entry_matches_the_abi(monkeypatch):
    """ops.text_attention: the packed tensor, three dense tensors and three band views give the kernel's result bit for bit and note
    `causal_fused`; a host tensor raises; "lib" and an unserved head size note `lib_core` and agree to rounding."""
    from stablekeypoints_amd import ops, routes
    c = T.case("randn", 2, 3, 77, 64)
    want = _run_kernel(c, "packed")
    assert torch.equal(_run_kernel(c, "padded"), want) and torch.equal(_run_kernel(c, "dense"), want)     # one arithmetic, three strides
    qkv = torch.cat([c.q, c.k, c.v], dim=-1).cuda()
    C = c.q.shape[-1]
    before = routes.snapshot()
    a = ops.text_attention(qkv, None, None, 3, c.scale)
    b = ops.text_attention(c.q.cuda(), c.k.cuda(), c.v.cuda(), 3, c.scale)
    e = ops.text_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], 3, c.scale)
    assert routes.delta(before) == {("text.attention", "causal_fused"): 3}
    for x in (a, b, e):
        assert torch.equal(x.cpu(), want)
    with pytest.raises(RuntimeError):
        ops.text_attention(c.q, c.k, c.v, 3, c.scale)
    assert ops.text_attn_supported(768, 12, 77) and ops.text_attn_supported(96, 3, 77)
    assert not ops.text_attn_supported(80, 2, 77) and not ops.text_attn_supported(768, 12, 129)
    monkeypatch.setattr(ops, "TEXT_ATTN_MODE", "lib")
    before = routes.snapshot()
    lib = ops.text_attention(qkv, None, None, 3, c.scale)
    assert routes.delta(before) == {("text.attention", "lib_core"): 1}
    A.assert_attn_close({"out": lib.cpu()}, c, 8, "text-attn lib_core")
    monkeypatch.setattr(ops, "TEXT_ATTN_MODE", "auto")
    before = routes.snapshot()
    ops.text_attention(torch.randn(1, 20, 3 * 80, device="cuda"), None, None, 2, 0.1)          # d = 40: no kernel
    assert routes.delta(before) == {("text.attention", "lib_core"): 1}


# ---------------------------------------------------------------------------------------------------------------------
# towers
# ---------------------------------------------------------------------------------------------------------------------
TOWERS = {"w128-d64": dict(width=128, heads=2, act="quick_gelu", projection_dim=64),
          "w96-d32": dict(width=96, heads=3, act="gelu")}


@pytest.mark.parametrize("name", list(TOWERS))
def test_tower_routes_and_accuracy(name, monkeypatch):
    import copy
    from stablekeypoints_amd import ops, routes
    cpu = T.tower(**TOWERS[name])
    ids = T.prompt_ids()
    ref64 = [copy.deepcopy(cpu).double()(ids, penultimate=p) for p in (False, True)]
    ref32 = [cpu(ids, penultimate=p) for p in (False, True)]
    gpu = copy.deepcopy(cpu).cuda()
    layers = len(gpu.text_model.encoder.layers)
    before = routes.snapshot()
    with routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
        got = [gpu(ids.cuda(), penultimate=p) for p in (False, True)]
    torch.cuda.synchronize()
    # per encode: one causal core per layer; the first norm + two residual-plus-norm joints per layer
    assert routes.delta(before) == {("text.attention", "causal_fused"): 2 * layers, ("add_layer_norm", "add_ln"): 2 * (2 * layers + 1)}
    worst = 0.0
    for g, r64, r32, what in ((got[0][0], ref64[0][0], ref32[0][0], "last"), (got[1][0], ref64[1][0], ref32[1][0], "penultimate"),
                              (got[0][1], ref64[0][1], ref32[0][1], "pooled")):
        assert g.shape == r64.shape and bool(torch.isfinite(g).all())
        err, e32 = A.rel_err(g.cpu(), r64), A.rel_err(r32, r64)
        assert e32 > 0
        print(f"text-tower {name} {what}: err {err:.3e} fp32 cpu tree {e32:.3e} ratio {err / e32:.2f}")
        worst = max(worst, err / e32)
        assert err <= T.M_TREE * e32 + A.ABS_SLACK, f"{name} {what}: err {err:.3e} > {T.M_TREE} x {e32:.3e}"
    # the library route: noted as such, refused by the strict block, same values to rounding
    monkeypatch.setattr(ops, "TEXT_ATTN_MODE", "lib")
    before = routes.snapshot()
    lib = gpu(ids.cuda())[0]
    assert routes.delta(before)[("text.attention", "lib_core")] == layers
    assert A.rel_err(lib.cpu(), ref64[0][0]) <= 8 * A.rel_err(ref32[0][0], ref64[0][0]) + A.ABS_SLACK
    with pytest.raises(routes.UnexpectedRoute):
        with routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
            gpu(ids.cuda())


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_uncond_prompt_end_to_end():
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, ctrls, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True, text_encoder=True)
    plain, pctrls, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True)
    ctrl, pctrl = next(iter(ctrls.values())), next(iter(pctrls.values()))
    emb = torch.randn(1, 77, 768, generator=torch.Generator().manual_seed(3))
    lat = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    kw = dict(num_inference_steps=2, latent=lat, height=64, width=64)
    unc = ptp_utils.encode_prompt(ldm, [""])
    assert unc.shape == (1, 77, 768) and unc.is_cuda
    a, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, uncond_prompt="", **kw)
    b, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, uncond_embedding=unc, **kw)
    assert (a == b).all()
    c, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, **kw)
    d, _ = ptp_utils.text2image_ldm_stable(plain, emb, pctrl, **kw)
    assert (c == d).all()
    assert (a != c).any(), "guidance against CLIP(\"\") changed nothing"
