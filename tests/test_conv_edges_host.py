"""CPU half of the convolution-edge tests: the input families of tests/_conv_cases.py have their stated property at every shape
the GPU tests use, every variant's shape reaches the launch plan it is listed for (the library's host queries and the restated
grid agree), and the checker the GPU tests assert with rejects a subtly wrong result at the tolerance they use.  For the kinds
`s2w`, `up2`, `out` and `in_fn` also: the polyphase emulations in fp64 are the convolution, the image reference clamps at both
ends and not at all, and the defects those forms make possible are rejected.  Nothing here touches a kernel."""
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
    # the polyphase stride-2 kernel
    assert has("s2w", tiles=1, ntb=1, ncg=1, groups=1)
    assert has("s2w", tiles=6, images_in_a_block=3, groups=2)
    assert has("s2w", tiles=27, ntb=2, ragged_tb=True, ncg=2, idle_ids=True) and not A.BY_NAME["s2w-two-cg-ragged-tb"]["bias"]
    assert has("s2w", stats_ok=True, groups=3) and A.BY_NAME["s2w-stats-one-block"]["stats"]
    assert has("s2w", groups=8) and A.BY_NAME["s2w-128-channels"]["shape"][1] == 128
    assert has("s2w", ntb=40, order="unit", ids=320, launched=256, persistent=True, stats_ok=True) and A.BY_NAME["s2w-unit-second-unit"]["stats"]
    assert has("s2w", ntb=65, order="banded", tb_per_xcd=9, ragged_band=True, persistent=False)
    assert has("s2w", ntb=260, order="banded", ids=264, persistent=True)
    assert all(v["pad"] == 0 and v["tune"] == {"conv_s2w": 1} and v["routed"] == ("conv3x3_s2", "s2_wino") for v in A.VARIANTS if v["kind"] == "s2w")
    # the up-sampling kernel
    assert has("up2", grid=(1, 1), ragged_y=True, ragged_x=True) and A.BY_NAME["up2-one-pixel"]["shape"][3:] == (1, 1)
    assert has("up2", grid=(2, 1), ragged_y=True, ragged_x=True)
    assert has("up2", tiles_y=2, tiles_x=2, stages=2, grid=(4, 2)) and A.BY_NAME["up2-seam-9x17"]["shape"][3:] == (9, 17)
    assert has("up2", tiles_x=13, ragged_x=True)
    assert has("up2", grid=(12, 3), stages=3, ragged_y=False, ragged_x=False) and not A.BY_NAME["up2-exact-tiles"]["bias"]
    assert all(v["tune"] == {"conv_up2": 1} and v["routed"] == ("upsample_conv", "up2_poly") for v in A.VARIANTS if v["kind"] == "up2")
    # the small-output kernel and ConvInFn
    assert has("out", Cout=1, blocks=1) and A.BY_NAME["out-1ch-1x2"]["shape"][3:] == (1, 2)
    assert has("out", Cout=2, blocks=1) and A.BY_NAME["out-2ch-5x6"]["shape"][0] == 2 and A.BY_NAME["out-2ch-5x6"]["shape"][3] % 2 == 1
    assert has("out", Cout=3, blocks=1, ragged_block=True)
    assert has("out", Cout=4, stages=3) and not A.BY_NAME["out-4ch-48"]["bias"]
    assert has("out", Cout=3, blocks=3, ragged_block=True)
    v3 = A.BY_NAME["out-3ch-three-blocks"]                 # pair 256, the first of the second block, is (row 11, column 28): mid-row
    assert divmod(256, v3["shape"][4] // 2) == (11, 14) and {(0, 11, 27), (0, 11, 28)} <= set(A.impulse_sites(1, 24, 44, v3["seam"]))
    assert any(v["kind"] == "in_fn" and v["bwd"] and v["routed"] == {("conv_in", "small"): 1, ("conv_in.bwd_data", "small_out"): 1}
               for v in A.VARIANTS)
    for v in A.VARIANTS:
        if v["kind"] in ("s2w", "up2", "out", "in_fn"):      # their own tile counts (s2w: 4x4 outputs, up2: 8x16 inputs, out: blocks)
            assert set(v["families"]) == set(A.FAMILIES if v["tiles"] <= 1000 else A.BIG_FAMILIES)
            continue
        tiles = v["shape"][0] * (v["shape"][3] // 4) * (v["shape"][4] // 4)
        assert set(v["families"]) == set(A.FAMILIES if (tiles <= 1000 or v["kind"] in ("small", "s2", "s2_fn", "f2")) else A.BIG_FAMILIES)


def test_image_reference_clamps_at_both_ends_and_not_at_all():
    """What makes the image epilogue visible: on dc, outlier and post_silu the fp64 image of every out-* shape but 1 x 2 has
    pixels clamped to 0, pixels clamped to 1 and pixels strictly inside (on randn-sized outputs a clamp applied before the scale,
    or not at all, moves few pixels)."""
    for v in A.VARIANTS:
        if v["kind"] != "out" or v["shape"][3:] == (1, 2):
            continue
        for family in ("dc", "outlier", "post_silu"):
            c = A.case(v, family)
            z = c.ref64["y"] / 2 + 0.5
            lo, hi, inside = int((z < 0).sum()), int((z > 1).sum()), int(((c.img64 > 0) & (c.img64 < 1)).sum())
            print(f"{v['name']} {family}: {lo} pixels clamped to 0, {hi} to 1, {inside} inside")
            assert lo > 0 and hi > 0 and inside > 0, (v["name"], family)
            assert bool((c.img64[z < 0] == 0).all()) and bool((c.img64[z > 1] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# the checker rejects planted defects
# ---------------------------------------------------------------------------------------------------------------------
DEFECT_VARIANT = A.BY_NAME["f4-c64-uneven-forced-S4"]        # (2, 112, 64, 16, 16): bias, residual, backward, splits of 2, 2, 2, 1 stages
TOLERANCES = sorted(set(A.M.values()) | {8})                 # (8: the cap of the rule the values of M follow)
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
    for name in ("f4-c64-uneven-forced-S4", "f2-v1-odd-33x17", "s2-fn-pad0", "small-3ch-128", "s2w-stats-one-block", "up2-seam-9x17",
                 "out-3ch-three-blocks", "in-fn-4ch"):
        v = A.BY_NAME[name]
        for family in ("randn", "dc", "outlier"):
            c = A.case(v, family)
            A.assert_conv_close(_exact(c), c, "fp64 itself", m=m)
            A.assert_conv_close(c.ref32, c, "fp32 reference", m=1)
            if v["kind"] in ("f4", "f2"):                 # the emulation itself, in fp64: the algorithm is the convolution
                e = A.winograd_emulate(c.x, c.w, c.bias, c.res, m=4 if v["kind"] == "f4" else 2, dtype=torch.float64)
                A.assert_conv_close({"y": e}, c, "emulation in fp64", m=m)
                assert A.plane_err(e, c.ref64["y"]) < 1e-12
            if v["kind"] in ("s2w", "up2"):
                e = (A.s2w_emulate if v["kind"] == "s2w" else A.up2_emulate)(c.x, c.w, c.bias, dtype=torch.float64)
                A.assert_conv_close({"y": e}, c, "emulation in fp64", m=m)
                assert A.plane_err(e, c.ref64["y"]) < 1e-12
                assert c.err32["y"] > 0
            if v["kind"] == "out":
                A.assert_image_close(c.ref32["y"], A.image_map(c.ref32["y"]), c, "fp32 reference", m=1)


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


# ---------------------------------------------------------------------------------------------------------------------
# the kernels of image sampling: emulations in fp64, and the defects their forms make possible
# ---------------------------------------------------------------------------------------------------------------------
POLYPHASE = [v for v in A.VARIANTS if v["kind"] in ("s2w", "up2")]


@pytest.mark.parametrize("v", POLYPHASE, ids=[v["name"] for v in POLYPHASE])
def test_polyphase_emulation_in_fp64_is_the_convolution(v):
    """The algorithm the fp32 reference runs -- polyphase F(4x4,2x2) with the phase filters (w0,w2) / (w1,0), or the four folded 2x2
    phase convolutions of the up-sampler -- is the convolution: in fp64 it matches F.conv2d below 1e-12 per plane, at every shape
    used; in fp32 its error is never zero (it divides the kernel's)."""
    c = A.case(v, "randn")
    e = (A.s2w_emulate if v["kind"] == "s2w" else A.up2_emulate)(c.x, c.w, c.bias, dtype=torch.float64)
    err = A.plane_err(e, c.ref64["y"])
    print(f"{v['name']}: emulation in fp64 {err:.1e}, in fp32 {c.err32['y']:.1e}")
    assert e.dtype == torch.float64 and err < 1e-12 and c.err32["y"] > 0


NEW_DEFECTS = {
    "s2w-stats-one-block": ["right_extension_reads_next_row", "bottom_extension_reads_next_channel", "skipped_block_multiplied_stale",
                            "row_and_column_phase_swapped_in_one_tile", "one_group_dropped_in_one_plane"],
    "up2-seam-9x17": ["border_replicated_not_zero", "row_phases_swapped", "ragged_tile_column_dropped", "stage_from_previous_patch"],
    "out-3ch-three-blocks": ["left_neighbour_wraps_to_previous_row", "second_pixel_of_pair_duplicated", "clamp_before_scale"],
    "in-fn-4ch": ["flipped_not_transposed_filter"],
}
NEW_DEFECT_CASES = [(name, d, f) for name, ds in NEW_DEFECTS.items() for d in ds for f in ("randn", "dc", "outlier")]


def _flat_shift(x, by):
    """x read `by` floats further on in its own flat NCHW buffer (zeros beyond both ends): what a load at a valid address past a
    row's or a plane's end returns."""
    flat = x.flatten()
    z = torch.zeros(abs(by), dtype=x.dtype)
    return (torch.cat([flat[by:], z]) if by > 0 else torch.cat([z, flat[:by]])).view_as(x)


def plant_new(defect, c):
    """The fp64 reference of case `c` (kinds s2w, up2, out, in_fn) with ONE defect; `out`: y in fp32 and the image made from it."""
    v = c.v
    B, ci, co, H, W = v["shape"]
    got = _exact(c)
    y, x, w = got["y"], c.x.double(), c.w.double()
    bias = None if c.bias is None else c.bias.double()
    quiet = divmod(int(A.plane_maxima(c.ref64["y"]).flatten().argmin()), co)
    # ---- s2w
    if defect == "right_extension_reads_next_row":        # column W of the (0,1,0,1) extension: the next address, not 0
        xe = F.pad(x, (0, 1, 0, 1))
        xe[:, :, :H, W] = _flat_shift(x, 1)[:, :, :, W - 1]
        y[:] = F.conv2d(xe, w, bias, stride=2)
    elif defect == "bottom_extension_reads_next_channel":  # row H: the first row of the next plane
        xe = F.pad(x, (0, 1, 0, 1))
        xe[:, :, H, :W] = _flat_shift(x, W)[:, :, H - 1, :]
        y[:] = F.conv2d(xe, w, bias, stride=2)
    elif defect in ("skipped_block_multiplied_stale", "row_and_column_phase_swapped_in_one_tile"):
        Vs, Us = A.s2w_parts(c.x, c.w, torch.float64)
        if defect == "skipped_block_multiplied_stale":     # position (4, 2) of phase (1, 0) is a structural zero; its accumulator
            p, (b, k) = A.S2W_PHASES.index((1, 0)), quiet  # gets the product of the block before it, (3, 2), in one plane
            assert bool((Us[p][:, :, 4, :] == 0).all())
            Mm = A.s2w_products(Vs, Us)
            Mm[:, k, :, :, 4, 2] += torch.einsum("bctu,c->btu", Vs[p][..., 3, 2], Us[p][k, :, 3, 2])
        else:
            p, q = A.S2W_PHASES.index((0, 1)), A.S2W_PHASES.index((1, 0))
            Vs = [t.clone() for t in Vs]
            Vs[p][1, :, 1, 2], Vs[q][1, :, 1, 2] = Vs[q][1, :, 1, 2].clone(), Vs[p][1, :, 1, 2].clone()
            Mm = A.s2w_products(Vs, Us)
        y[:] = A.s2w_finish(Mm, bias)
    elif defect == "one_group_dropped_in_one_plane":       # the second 16-channel group of three, in the quietest plane
        b, k = quiet
        y[b, k] -= A.conv_s2(c.x[b:b + 1, 16:32], c.w[k:k + 1, 16:32], None, 0, torch.float64)[0, 0]
    # ---- up2
    elif defect == "border_replicated_not_zero":           # the low-resolution index clamped: edge replication of the up-sampled image
        up = F.interpolate(x, scale_factor=2, mode="nearest")
        y[:] = F.conv2d(F.pad(up, (1, 1, 1, 1), mode="replicate"), w, bias)
    elif defect == "row_phases_swapped":
        y[:] = c.ref64["y"].reshape(B, co, H, 2, 2 * W).flip(3).reshape(B, co, 2 * H, 2 * W)
    elif defect == "ragged_tile_column_dropped":           # the last valid low-resolution column: its output pair is left at the bias
        y[:, :, :, 2 * W - 2:] = bias[None, :, None, None]
    elif defect == "stage_from_previous_patch":            # stage 1 of the first tile multiplies stage 0's patch
        wrong = A.up2_ref(c.x[:, 0:16], c.w[:, 16:32], None) - A.up2_ref(c.x[:, 16:32], c.w[:, 16:32], None)
        y[:, :, :16, :32] += wrong[:, :, :16, :32]
    # ---- out
    elif defect == "left_neighbour_wraps_to_previous_row":  # row[-1] at x0 = 0 is the previous row's last pixel
        xp = F.pad(x, (1, 1, 1, 1))
        xp[:, :, 1:H + 1, 0] = _flat_shift(x, -1)[:, :, :, 0]
        y[:] = F.conv2d(xp, w, bias)
    elif defect == "second_pixel_of_pair_duplicated":
        y[:, :, :, 1::2] = c.ref64["y"][:, :, :, 0::2]
    elif defect == "flipped_not_transposed_filter":        # the flipped filter read as [Cin, Cout, 3, 3] without the transpose
        got["dx"] = F.conv2d(c.dy.double(), w.flip(2, 3).contiguous().view(ci, co, 3, 3), padding=1)
    else:
        raise KeyError(defect)
    return got


@pytest.mark.parametrize("m", TOLERANCES)
@pytest.mark.parametrize("name,defect,family", NEW_DEFECT_CASES, ids=[f"{d}-{f}" for _, d, f in NEW_DEFECT_CASES])
def test_checker_rejects_planted_defect_of_the_sampling_kernels(name, defect, family, m):
    """As test_checker_rejects_planted_defect, for the failures the polyphase stride-2, the up-sampling and the small-output
    kernels can have; printed: whether the bound their earlier tests use, assert_close(rtol 1e-4, atol 2e-5 x max|ref|) over the
    whole tensor, would have let it pass (profiles/conv_edges.md)."""
    c = A.case(A.BY_NAME[name], family)
    if defect == "clamp_before_scale":                     # on the image: y itself is right (the fp32 reference)
        y = c.ref32["y"]
        img = y.clamp(0, 1) * 0.5 + 0.5
        old = A.whole_tensor_bound_accepts(img, c.img64, atol=2e-5)
        print(f"conv-defect {defect} {family}: largest |img - img64| {(img.double() - c.img64).abs().max().item():.3e}, "
              f"whole-tensor bound {'ACCEPTS' if old else 'rejects'}")
        A.assert_image_close(y, A.image_map(y), c, "the right image", m=m)
        bad = A.image_errors(y, img, c, m=m)
        assert len(bad) == 2, "both the bit comparison and the derived bound must reject it"
        with pytest.raises(AssertionError):
            A.assert_image_close(y, img, c, defect, m=m)
        return
    got = plant_new(defect, c)
    out = "dx" if defect == "flipped_not_transposed_filter" else "y"
    assert not torch.equal(got[out], c.ref64[out])
    old = A.whole_tensor_bound_accepts(got[out], c.ref64[out], atol=2e-5)
    print(f"conv-defect {defect} {family}: plane err {A.plane_err(got[out], c.ref64[out]):.3e}, fp32ref {c.err32[out]:.3e}, "
          f"whole-tensor bound {'ACCEPTS' if old else 'rejects'}")
    with pytest.raises(AssertionError):
        A.assert_conv_close(got, c, defect, m=m)
