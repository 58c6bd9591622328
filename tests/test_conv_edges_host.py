"""CPU half of the convolution-edge tests: the input families of tests/_conv_cases.py have their stated property at every shape
the GPU tests use, every variant's shape reaches the launch plan it is listed for (the library's host queries and the restated
grid agree), and the checker the GPU tests assert with rejects a subtly wrong result at the tolerance they use.  Nothing here
touches a kernel."""
import pytest
import torch
import torch.nn.functional as F

import _conv_cases as A

CASES = [(v, f) for v in A.VARIANTS for f in v["families"]]


@pytest.mark.parametrize("v,family", CASES, ids=[f"{v['name']}-{f}" for v, f in CASES])
def test_family_has_its_property_at_every_shape_used(v, family):
    """The family's property on x (and on dy where the variant has a backward launch); every reference finite; no output
    identically zero; every fp64 output plane's maximum at least 1e-2 of the global one (the per-plane error divides by it)."""
    c = A.case(v, family)
    for t, seam in ((c.x, v["seam"]), (c.dy, v["seam_out"])):
        if t is not None:
            ok, what = A.check_property(family, t, seam)
            print(f"{v['name']} {family} {tuple(t.shape)}: {what}")
            assert ok, f"{family} at {tuple(t.shape)}: {what}"
    found = A.input_conditions(c)
    print(f"{v['name']} {family}: smallest plane maximum / global maximum " + ", ".join(f"{k} {x:.2f}" for k, x in found.items()))


def test_impulse_output_is_the_rotated_filter():
    """What the impulse family pins down: around an impulse of value a in channel k at (i, j), output channel c holds
    a * w[c, k] rotated by 180 degrees (cut off at the border) -- in the fp64 reference the kernels are compared with."""
    v = dict(A.BY_NAME["f4-c64-one-block"], bias=False, res=False, bwd=False, name="impulse-alone")
    c = A.Case(v, "impulse")
    B, ci, co, H, W = v["shape"]
    for i, (b, yy, xx) in enumerate(A.impulse_sites(B, H, W, v["seam"])):
        k, a = i % ci, 1.0 + 0.25 * i
        alone = torch.zeros(1, ci, H, W, dtype=torch.float64)
        alone[0, k, yy, xx] = a
        y = F.conv2d(alone, c.w.double(), padding=1)[0]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= yy + dy < H and 0 <= xx + dx < W:
                    assert torch.equal(y[:, yy + dy, xx + dx], a * c.w[:, k, 1 - dy, 1 - dx].double())


@pytest.mark.parametrize("v", A.VARIANTS, ids=[v["name"] for v in A.VARIANTS])
def test_variant_shape_reaches_its_launch_plan(v, tune):
    """The table of variants against the restated plans and the library's own queries (host code of libskp_hip.so: no GPU needed;
    256 compute units assumed, the GPU tests take the count from the device)."""
    from stablekeypoints_amd import ops
    for key, value in v["tune"].items():
        tune(key, value)
    facts = A.assert_plan(ops, v, ncu=256)
    print(v["name"], v["shape"], facts)


def test_every_listed_property_is_reached():
    """Every launch property the table exists for is reached by at least one variant (each variant's own `reach` is proven by
    test_variant_shape_reaches_its_launch_plan)."""
    def has(kind, **want):
        return any(v["kind"] == kind and all(v["reach"].get(k) == x for k, x in want.items()) for v in A.VARIANTS)
    assert has("f4", form="c64", ntb=1, S=1) and has("f4", form="c64", images_in_a_block=3, ragged_cg=True, tiles=27)
    assert has("f4", form="c64", tiles=6, S=3) and has("f4", form="c64", order="banded", ragged_band=True, empty_xcd=True, ntb=33)
    assert has("f4", form="c128", ncg=1, S=1) and has("f4", form="c128", ncg=3, ragged_cg=True)
    assert has("f4", form="c128", ntb=9, ragged_tb=True, images_in_a_block=2, S=5)
    assert has("f4", form="c128", order="banded", persistent=True, ids=384) and has("f4", form="c128", order="banded", persistent=True, ids=272, ragged_band=True)
    assert has("f4", form="c128", order="unit", persistent=True, idle_ids=True, ids=320, units=36)
    assert has("f4", stages=(2, 2, 2, 1)) and has("f4", S=7) and has("f4", ids=256, launched=256, persistent=False)
    assert any(v["kind"] == "f4" and not v["split"] and v["reach"]["S"] > 1 for v in A.VARIANTS)
    assert has("f4_stats", form="c64") and has("f4_stats", form="c128")
    assert has("gn", ncg=1) and has("gn", ncg=3) and any(v["kind"] == "gn" and v["off"] and v["stats"] for v in A.VARIANTS)
    for tiles in (1, 32, 18, 12):
        assert has("f4r", tiles=tiles, S=1)
    assert has("f4r", stages=(9, 8)) and has("f4r", stages=(6, 6, 5)) and has("f4r", stages=(6, 6, 4)) and has("f4r", stages=(7, 7, 6))
    assert any(v["kind"] == "f4r" and v["bwd"] for v in A.VARIANTS)
    for variant in (1, 2):
        assert any(v["kind"] == "f2" and v["variant"] == variant and v["shape"][3] % 2 for v in A.VARIANTS)
        assert has("f2", variant=variant, ragged_cg=True)
    assert any(v["kind"] == "f2" and v["reach"]["S"] > 1 and v["split"] for v in A.VARIANTS)
    assert any(v["kind"] == "f2" and v["reach"]["S"] > 1 and not v["split"] for v in A.VARIANTS)
    for pad in (0, 1):
        assert any(v["kind"] == "s2" and v["pad"] == pad and not v["ws"] for v in A.VARIANTS)
        assert any(v["kind"] == "s2_fn" and v["pad"] == pad and v["bwd"] for v in A.VARIANTS)
    assert any(v["kind"] == "s2" and v["ws"] for v in A.VARIANTS)
    assert {v["shape"] for v in A.VARIANTS if v["kind"] == "small"} == {(3, 1, 5, 9, 2), (1, 4, 32, 8, 8), (2, 3, 128, 16, 32)}
    for v in A.VARIANTS:
        tiles = v["shape"][0] * (v["shape"][3] // 4) * (v["shape"][4] // 4)
        assert set(v["families"]) == set(A.FAMILIES if (tiles <= 1000 or v["kind"] in ("small", "s2", "s2_fn", "f2")) else A.BIG_FAMILIES)


# ---------------------------------------------------------------------------------------------------------------------
# the checker rejects planted defects
# ---------------------------------------------------------------------------------------------------------------------
DEFECT_VARIANT = A.BY_NAME["f4-c64-uneven-forced-S4"]        # (2, 112, 64, 16, 16): bias, residual, backward, splits of 2, 2, 2, 1 stages
TOLERANCES = sorted(set(A.M.values()))
DEFECTS = ["stage_dropped_in_one_plane", "tile_one_to_the_right", "filter_transposed_not_rotated", "bias_once_per_split",
           "bottom_row_edge_replicated", "last_image_from_the_previous"]
# one more, a numerical one: the inputs of ONE 16-channel stage of the 7 rounded to 11 mantissa bits (a matrix instruction of the
# wrong precision).  On randn -- the only inputs of the earlier tests -- their whole-tensor bound accepts it; the outlier family
# cannot show it (the large channel's own rounding is 10 x larger), so it runs on randn and dc.
DEFECT_CASES = [(d, f) for d in DEFECTS for f in ("randn", "dc", "outlier")] + [("one_stage_at_11_bits", "randn"), ("one_stage_at_11_bits", "dc")]


def _exact(c):
    return {name: x.clone() for name, x in c.ref64.items()}


@pytest.mark.parametrize("m", TOLERANCES)
def test_checker_accepts_the_references(m):
    for name in ("f4-c64-uneven-forced-S4", "f2-v1-odd-33x17", "s2-fn-pad0", "small-3ch-128"):
        v = A.BY_NAME[name]
        for family in ("randn", "dc", "outlier"):
            c = A.case(v, family)
            A.assert_conv_close(_exact(c), c, "fp64 itself", m=m)
            A.assert_conv_close(c.ref32, c, "fp32 reference", m=1)
            if v["kind"] in ("f4", "f2"):                 # the emulation itself, in fp64: the algorithm is the convolution
                e = A.winograd_emulate(c.x, c.w, c.bias, c.res, m=4 if v["kind"] == "f4" else 2, dtype=torch.float64)
                A.assert_conv_close({"y": e}, c, "emulation in fp64", m=m)
                assert A.plane_err(e, c.ref64["y"]) < 1e-12


def plant(defect, c):
    """The fp64 reference of case `c` with ONE defect."""
    v = c.v
    B, ci, co, H, W = v["shape"]
    got = _exact(c)
    y = got["y"]
    if defect == "stage_dropped_in_one_plane":            # the last 16-channel stage of the first K split, in the quietest plane
        b, k = divmod(int(A.plane_maxima(c.ref64["y"]).flatten().argmin()), co)
        k0 = 16 * (v["reach"]["stages"][0] - 1)
        y[b, k] -= F.conv2d(c.x[b:b + 1, k0:k0 + 16].double(), c.w[k:k + 1, k0:k0 + 16].double(), padding=1)[0, 0]
    elif defect == "tile_one_to_the_right":
        y[1, 5, 4:8, 8:12] = c.ref64["y"][1, 5, 4:8, 4:8]
    elif defect == "filter_transposed_not_rotated":
        got["dx"] = F.conv2d(c.dy.double(), c.w.transpose(0, 1).double(), padding=1)
    elif defect == "bias_once_per_split":
        y += (v["reach"]["S"] - 1) * c.bias.double()[None, :, None, None]
    elif defect == "bottom_row_edge_replicated":
        xp = F.pad(F.pad(c.x.double(), (1, 1, 1, 0)), (0, 0, 0, 1), mode="replicate")
        xp[:, :, -1, 0] = xp[:, :, -1, -1] = 0
        y[:] = F.conv2d(xp, c.w.double(), c.bias.double()) + c.res.double()
    elif defect == "last_image_from_the_previous":
        y[-1] = c.ref64["y"][-2]
    elif defect == "one_stage_at_11_bits":
        k0 = 16 * (ci // 16 - 1)
        xs = c.x[:, k0:k0 + 16].double()
        mant, expo = torch.frexp(xs)
        y += F.conv2d(torch.ldexp(torch.round(mant * 2 ** 11) / 2 ** 11, expo) - xs, c.w[:, k0:k0 + 16].double(), padding=1)
    return got


@pytest.mark.parametrize("m", TOLERANCES)
@pytest.mark.parametrize("defect,family", DEFECT_CASES, ids=[f"{d}-{f}" for d, f in DEFECT_CASES])
def test_checker_rejects_planted_defect(defect, family, m):
    """The fp64 reference with ONE defect must fail `assert_conv_close` at the tolerance the GPU tests use; printed: whether the
    whole-tensor bound of the earlier tests (6e-5 x max|ref|) would have let it pass (profiles/conv_edges.md)."""
    c = A.case(DEFECT_VARIANT, family)
    got = plant(defect, c)
    name = "dx" if defect == "filter_transposed_not_rotated" else "y"
    assert not torch.equal(got[name], c.ref64[name])
    old = A.whole_tensor_bound_accepts(got[name], c.ref64[name])
    print(f"conv-defect {defect} {family}: plane err {A.plane_err(got[name], c.ref64[name]):.3e}, fp32ref {c.err32[name]:.3e}, "
          f"whole-tensor bound {'ACCEPTS' if old else 'rejects'}")
    with pytest.raises(AssertionError):
        A.assert_conv_close(got, c, defect, m=m)
    if (defect, family) == ("one_stage_at_11_bits", "randn"):
        assert old, "the earlier bound was expected to let this one pass"
