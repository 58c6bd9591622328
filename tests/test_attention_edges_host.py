"""CPU half of the attention-edge tests: the input families of tests/_attn_cases.py really are hard (their fp64 logits have the
stated property at every shape the GPU tests use), and the checker the GPU tests assert with rejects a subtly wrong result
at the tolerance they use.  Nothing here touches a kernel."""
import pytest
import torch

import _attn_cases as A

SHAPES = sorted({(v["shape"], f) for v in A.VARIANTS for f in v["families"]}, key=lambda sf: (sf[0][5], sf[0], A.FAMILIES.index(sf[1])))


@pytest.mark.parametrize("shape,family", SHAPES, ids=[f"{'x'.join(map(str, s))}-{f}" for s, f in SHAPES])
def test_family_has_its_property_at_every_shape_used(shape, family):
    """Conditions on the inputs, in fp64: the family's logit property; every reference output finite; no gradient identically zero."""
    c = A.case(family, *shape)
    d = shape[5]
    ok, what = A.check_property(family, c.logits(), d, c.scale)
    print(f"{family} {shape}: {what}")
    assert ok, f"{family} at (B,Bk,H,N,Nk,d)={shape}: {what}"
    assert float(torch.tensor(c.scale, dtype=torch.float32)) == c.scale          # fp32 holds the scale exactly
    for name, x in c.ref64.items():
        assert torch.isfinite(x).all(), name
    for name in ("dq", "dk", "dv"):
        assert c.ref64[name].abs().max().item() > 0, name
    for t in (c.q, c.k, c.v, c.dout):
        assert t.dtype == torch.float32 and torch.isfinite(t).all()


@pytest.mark.parametrize("v", A.VARIANTS, ids=[v["name"] for v in A.VARIANTS])
def test_variant_shape_reaches_its_launch_plan(v, tune):
    """The table of variants against the restated gates and the library's own queries (host code of libskp_hip.so: no GPU needed)."""
    from stablekeypoints_amd import ops
    for key, value in v["tune"].items():
        tune(key, value)
    A.assert_plan(ops, v)


# ---------------------------------------------------------------------------------------------------------------------
# the checker rejects planted defects
# ---------------------------------------------------------------------------------------------------------------------
DEFECT_SHAPE = (2, 1, 2, 130, 200, 40)          # B, Bk, H, N, Nk, d: shared k / v, ragged query and key tiles
TOLERANCES = sorted(set(A.M.values()))


def _exact(c):
    return {name: x.clone() for name, x in c.ref64.items()}


def _online_out(c, tile=64, skip_rescale_when_max_rises=False):
    """Key-tiled online softmax in fp64, as the flash kernels run it; the defect keeps the accumulator as it is in a tile that
    raises the running maximum (the row sum is rescaled correctly)."""
    H = c.H
    S = c.logits()
    vh = A._split(c.v, H, torch.float64)
    m = torch.full(S.shape[:-1] + (1,), -float("inf"), dtype=torch.float64)
    l = torch.zeros_like(m)
    acc = torch.zeros(S.shape[:-1] + (vh.shape[-1],), dtype=torch.float64)
    for j in range(0, S.shape[-1], tile):
        s = S[..., j:j + tile]
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        keep = alpha if not (skip_rescale_when_max_rises and j > 0) else torch.where(m_new > m, torch.ones_like(alpha), alpha)
        acc = acc * keep + p @ vh[..., j:j + tile, :]
        m = m_new
    return A._merge(acc / l)


@pytest.mark.parametrize("m", TOLERANCES)
def test_checker_accepts_the_references(m):
    for family in ("randn", "ramp_up", "all_high", "odd_scale"):
        c = A.case(family, *DEFECT_SHAPE)
        A.assert_attn_close(_exact(c), c, m, "fp64 itself")
        A.assert_attn_close(c.ref32, c, 1, "fp32 reference")
        A.assert_attn_close({"out": _online_out(c)}, c, m, "online softmax emulation without the defect")


@pytest.mark.parametrize("m", TOLERANCES)
@pytest.mark.parametrize("defect", ["last_key_dropped", "head_size_scale", "lse_shifted", "dk_row_repeated", "tile_not_rescaled"])
def test_checker_rejects_planted_defect(defect, m):
    """The fp64 reference with ONE defect must fail `assert_attn_close` at the tolerance the GPU tests use."""
    family = {"head_size_scale": "odd_scale", "tile_not_rescaled": "ramp_up"}.get(defect, "randn")
    c = A.case(family, *DEFECT_SHAPE)
    B, Bk, H, N, Nk, d = DEFECT_SHAPE
    got = _exact(c)
    if defect == "last_key_dropped":
        r = A.reference(c.q, c.k[:, :-1], c.v[:, :-1], c.dout, c.scale, H, torch.float64)
        zero = torch.zeros(B, 1, H * d, dtype=torch.float64)
        got = {"out": r["out"], "lse": r["lse"], "dq": r["dq"], "dk": torch.cat([r["dk"], zero], 1), "dv": torch.cat([r["dv"], zero], 1)}
    elif defect == "head_size_scale":
        got = A.reference(c.q, c.k, c.v, c.dout, d ** -0.5, H, torch.float64)
    elif defect == "lse_shifted":
        got["lse"] += 1e-4
    elif defect == "dk_row_repeated":
        got["dk"][1] = got["dk"][0]
    elif defect == "tile_not_rescaled":
        got["out"] = _online_out(c, skip_rescale_when_max_rises=True)
    with pytest.raises(AssertionError):
        A.assert_attn_close(got, c, m, defect)
    if defect == "dk_row_repeated":               # the summed gradient alone is what the suite checked before
        assert "dk:" in _failure(got, c, m)


def _failure(got, c, m):
    try:
        A.assert_attn_close(got, c, m, "")
    except AssertionError as e:
        return str(e)
    return ""
