"""The polyphase Winograd F(4x4,2x2) form of the 3x3 / stride-2 convolution (csrc/skp_conv_s2w.hip) on the MI355X: parity with
fp64, padding and phase indexing, determinism, the block statistics its epilogue leaves for the next GroupNorm, the module
route with its gate, and the argument checks of its C entries.  Every test forces the route with the `conv_s2w` tune key, so the
small shapes here take the new kernel whatever the measured gate says."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

F = torch.nn.functional


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def _ref64(x, w, b, pad):
    xd = x.double()
    if pad == 0:
        return F.conv2d(F.pad(xd, (0, 1, 0, 1)), w.double(), None if b is None else b.double(), stride=2)
    return F.conv2d(xd, w.double(), None if b is None else b.double(), stride=2, padding=1)


def _case(B, ci, co, H, W, bias, seed=31):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    b = torch.randn(co, generator=g) if bias else None
    return x, w, b


def _run(ops, tune, x, w, b, pad, route, want_stats=False):
    """conv3x3_s2 with the route forced: 1 = polyphase Winograd, 2 = direct; checks the ledger noted that route."""
    from stablekeypoints_amd import routes
    tune("conv_s2w", route)
    before = routes.snapshot()
    with torch.no_grad():
        y = ops.conv3x3_s2(x, w, b, pad=pad, want_stats=want_stats)
    d = routes.delta(before)
    assert d.get(("conv3x3_s2", "s2_wino" if route == 1 else "s2_direct"), 0) == 1 and sum(d.values()) == 1
    return y


# one stage per phase; the step's smallest-channel form; two channel groups, tile count no multiple of 16, odd batch; more work
# units than workgroups in the unit-grouped order (40 tile blocks: persistent workgroups walk on to a second unit); the XCD-banded
# order with a ragged band (260 tile blocks) and second units
@pytest.mark.parametrize("B,ci,co,H,W,bias", [(1, 16, 128, 32, 64, True), (2, 128, 128, 64, 64, True), (3, 32, 256, 48, 96, False),
                                              (2, 16, 128, 128, 160, True), (1, 16, 128, 512, 520, True)])
def test_s2w_vs_fp64_and_deterministic(ops, tune, B, ci, co, H, W, bias):
    x, w, b = _case(B, ci, co, H, W, bias)
    ref = _ref64(x, w, b, 0)
    xg, wg, bg = x.cuda(), w.cuda(), None if b is None else b.cuda()
    assert ops.N.lib().skp_conv3x3_s2w_ok(B, ci, co, H, W, 0) in (0, 1)
    y = _run(ops, tune, xg, wg, bg, 0, 1)
    y2 = _run(ops, tune, xg, wg, bg, 0, 1)
    assert y.shape == ref.shape
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())
    assert torch.equal(y, y2)                                   # no K split, no atomics: the same bits


def test_s2w_gate_refuses_what_the_kernel_cannot_run(ops, tune):
    """Symmetric padding 1 (the UNet's layers) and a ragged last channel group stay on the direct kernel even when the route is
    forced, and the direct kernel still serves them."""
    lib = ops.N.lib()
    tune("conv_s2w", 1)
    assert lib.skp_conv3x3_s2w_ok(1, 48, 128, 32, 32, 1) == 0
    assert lib.skp_conv3x3_s2w_ok(1, 64, 192, 32, 64, 0) == 0
    assert lib.skp_conv3x3_s2w_ok(1, 64, 128, 32, 64, 0) == 1
    assert lib.skp_conv3x3_s2w_ok(1, 24, 128, 32, 64, 0) == 0 and lib.skp_conv3x3_s2w_ok(1, 64, 128, 36, 64, 0) == 0
    tune("conv_s2w", 2)
    assert lib.skp_conv3x3_s2w_ok(1, 64, 128, 32, 64, 0) == 0
    tune("conv_s2w", 1)
    for (B, ci, co, H, W, pad) in ((1, 48, 128, 32, 32, 1), (1, 64, 192, 32, 64, 0)):
        x, w, b = _case(B, ci, co, H, W, True, seed=5)
        from stablekeypoints_amd import routes
        before = routes.snapshot()
        with torch.no_grad():
            y = ops.conv3x3_s2(x.cuda(), w.cuda(), b.cuda(), pad=pad)
        assert routes.delta(before) == {("conv3x3_s2", "s2_direct"): 1}
        ref = _ref64(x, w, b, pad)
        torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())


def test_s2w_corner_and_edge_pixels(ops, tune):
    """One non-zero pixel at each image corner and on each edge (and one inside), distinct values, in distinct channels: the zero
    extension on the right / bottom, the phase a pixel belongs to and the tile it lands in."""
    B, ci, co, H, W = 2, 16, 128, 32, 64
    x = torch.zeros(B, ci, H, W)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 31), (H - 1, 32), (15, 0), (16, W - 1), (7, 8), (8, 7), (9, 9)]
    for n, (r, c) in enumerate(spots):
        x[n % B, n % ci, r, c] = 1.0 + 0.25 * n
    g = torch.Generator().manual_seed(3)
    w = torch.randn(co, ci, 3, 3, generator=g)
    b = torch.randn(co, generator=g)
    ref = _ref64(x, w, b, 0)
    y = _run(ops, tune, x.cuda(), w.cuda(), b.cuda(), 0, 1)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())


def test_s2w_block_statistics_merge_to_group_moments(ops, tune):
    """The epilogue's {mean, sum of squared deviations} per block of 16 consecutive 4x4 tiles: the blocks against torch (tolerances
    of the Winograd statistics test), and merged by the GroupNorm kernel that consumes them (skp_group_norm_fwd_blocks_f32) against
    the fp64 mean and variance of y per (image, group).  The output is the plain launch's, bit for bit."""
    B, ci, co, H, W, groups, eps = 2, 32, 128, 64, 128, 32, 1e-6
    x, w, b = _case(B, ci, co, H, W, True, seed=41)
    b = b * 3.0                                                  # means far from zero
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    y0 = _run(ops, tune, xg, wg, bg, 0, 1)
    y = _run(ops, tune, xg, wg, bg, 0, 1, want_stats=True)
    assert torch.equal(y, y0) and not hasattr(y0, "_skp_blocks")
    bs, nblk, pix = y._skp_blocks
    OH, OW = H // 2, W // 2
    assert (nblk, pix) == (OH * OW // 256, 256) and bs.shape == (B, co, nblk, 2)
    assert ops._blocks(y) is not None                            # the geometry the consumer accepts
    t = y.reshape(B, co, OH // 4, 4, OW // 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(B, co, nblk, 256).double()
    torch.testing.assert_close(bs[..., 0].double(), t.mean(-1), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bs[..., 1].double(), ((t - t.mean(-1, keepdim=True)) ** 2).sum(-1), rtol=1e-4, atol=1e-4)
    # merged by the consumer
    gamma, beta = torch.ones(co, device="cuda"), torch.zeros(co, device="cuda")
    z = torch.empty_like(y)
    mean = torch.empty(B, groups, device="cuda")
    rstd = torch.empty_like(mean)
    ops.N.check(ops.N.lib().skp_group_norm_fwd_blocks_f32(y.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), z.data_ptr(),
                                                          mean.data_ptr(), rstd.data_ptr(), bs.data_ptr(), nblk, pix, B, co, groups,
                                                          OH * OW, eps, 0, ops._stream()), "skp_group_norm_fwd_blocks_f32")
    yg = y.double().reshape(B, groups, -1)
    torch.testing.assert_close(mean.double(), yg.mean(-1), rtol=1e-5, atol=1e-6)
    var = rstd.double() ** -2 - eps
    torch.testing.assert_close(var, yg.var(-1, unbiased=False), rtol=1e-4, atol=1e-6)
    # a tile count per image that is no multiple of 16 leaves no block sums (blocks would straddle images) and still runs
    x2, w2, b2 = _case(3, 32, 128, 48, 96, True, seed=2)
    y2 = _run(ops, tune, x2.cuda(), w2.cuda(), b2.cuda(), 0, 1, want_stats=True)
    assert not hasattr(y2, "_skp_blocks")
    ref2 = _ref64(x2, w2, b2, 0)
    torch.testing.assert_close(y2.cpu().double(), ref2, rtol=1e-4, atol=2e-5 * ref2.abs().max().item())


# the smallest 128-channel launch the measured gate admits: 4096 tiles = one work unit per CU (s2w_shape_ok in csrc/skp_conv_s2w.hip)
GATED = (1, 128, 512, 512)


def test_downsample_module_takes_the_gated_route(ops, tune):
    """`Downsample2D(128, padding=0)`, frozen, under no_grad, after fuse_norms, with the library's own gate: equal to its eager
    forward; at a shape the gate admits the ledger shows `s2_wino` once, and `s2_direct` with the route forced off."""
    from stablekeypoints_amd import routes
    from stablekeypoints_amd.ldm.fused import fuse_norms
    from stablekeypoints_amd.ldm.unet import Downsample2D
    B, C, H, W = GATED
    assert ops.N.lib().skp_conv3x3_s2w_ok(B, C, C, H, W, 0) == 1, "the gate no longer admits the shape this test pins"
    assert ops.N.lib().skp_conv3x3_s2w_ok(B, C, C, H // 2, W, 0) == 0            # half a unit per CU: the direct kernel's
    torch.manual_seed(9)
    m = Downsample2D(C, padding=0).cuda()
    for p in m.parameters():
        p.requires_grad = False
    x = torch.randn(B, C, H, W, device="cuda")
    with torch.no_grad():
        eager = m(x)
        assert fuse_norms(m) == 1
        before = routes.snapshot()
        mine = m(x)
        d = routes.delta(before)
        assert d == {("downsample", "s2_direct"): 1, ("conv3x3_s2", "s2_wino"): 1}
        assert getattr(mine, "_skp_blocks", None) is not None and mine._skp_blocks[2] == 256
        tune("conv_s2w", 2)
        before = routes.snapshot()
        direct = m(x)
        assert routes.delta(before) == {("downsample", "s2_direct"): 1, ("conv3x3_s2", "s2_direct"): 1}
    tol = dict(rtol=1e-4, atol=2e-5 * eager.abs().max().item())
    torch.testing.assert_close(mine, eager, **tol)
    torch.testing.assert_close(direct, eager, **tol)


def test_s2w_error_ratio_recorded(ops, tune):
    """128 -> 128 @64^2: max |y - y64| / max |y64| of the Winograd form and of the direct kernel, printed (and written to
    SKP_S2W_ERR_OUT when set); both inside the parity tolerance -- that is the assertion."""
    x, w, b = _case(2, 128, 128, 64, 64, True)
    ref = _ref64(x, w, b, 0)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    scale = ref.abs().max().item()
    errs = {}
    for name, route in (("s2_wino", 1), ("s2_direct", 2)):
        y = _run(ops, tune, xg, wg, bg, 0, route)
        errs[name] = ((y.cpu().double() - ref).abs().max() / scale).item()
        torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * scale)
    line = "conv_s2w error ratio 128->128 @64^2 (max |y - y64| / max |y64|): " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
    print(line)
    out = os.environ.get("SKP_S2W_ERR_OUT")
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def test_s2w_c_abi_rejects_bad_arguments(ops):
    """Every refusal comes back as an error code before any launch (null pointers, sizes, padding, tile and channel multiples,
    statistics blocks that would straddle images)."""
    lib = ops.N.lib()
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    BAD, RANGE = -1, -2
    assert lib.skp_conv3x3_s2w_filter_f32(None, p, 128, 16, 0, None) == BAD
    assert lib.skp_conv3x3_s2w_filter_f32(p, None, 128, 16, 0, None) == BAD
    assert lib.skp_conv3x3_s2w_filter_f32(p, p, 0, 16, 0, None) == BAD
    assert lib.skp_conv3x3_s2w_filter_f32(p, p, 128, 16, 2, None) == BAD
    assert lib.skp_conv3x3_s2w_filter_f32(p, p, 128, 24, 0, None) == RANGE
    assert lib.skp_conv3x3_s2w_filter_f32(p, p, 4096, 4096, 0, None) == RANGE          # U past 2 GiB
    for fn in (lambda *a: lib.skp_conv3x3_s2w_f32(*a), lambda x, U, b, y, *a: lib.skp_conv3x3_s2w_stats_f32(x, U, b, y, p, *a)):
        assert fn(None, p, None, p, 1, 16, 128, 32, 64, 0, None) == BAD
        assert fn(p, None, None, p, 1, 16, 128, 32, 64, 0, None) == BAD
        assert fn(p, p, None, None, 1, 16, 128, 32, 64, 0, None) == BAD
        assert fn(p, p, None, p, 0, 16, 128, 32, 64, 0, None) == BAD
        assert fn(p, p, None, p, 1, 16, 128, 32, 64, 3, None) == BAD
        assert fn(p, p, None, p, 1, 16, 128, 32, 64, 1, None) == RANGE                  # symmetric padding: the direct kernel's
        assert fn(p, p, None, p, 1, 24, 128, 32, 64, 0, None) == RANGE
        assert fn(p, p, None, p, 1, 16, 192, 32, 64, 0, None) == RANGE
        assert fn(p, p, None, p, 1, 16, 128, 36, 64, 0, None) == RANGE
        assert fn(p, p, None, p, 1, 16, 128, 32, 68, 0, None) == RANGE
        assert fn(p, p, None, p, 64, 128, 128, 512, 512, 0, None) == RANGE              # x past 2 GiB
    assert lib.skp_conv3x3_s2w_stats_f32(p, p, None, p, None, 1, 16, 128, 32, 64, 0, None) == BAD
    assert lib.skp_conv3x3_s2w_stats_f32(p, p, None, p, p, 3, 32, 128, 48, 96, 0, None) == RANGE       # 72 tiles per image
    assert lib.skp_tune_get(b"conv_s2w") == 0
    torch.cuda.synchronize()
