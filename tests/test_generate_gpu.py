"""Image sampling on the MI355X: the up-sampling convolution (csrc/skp_conv_up2.hip) and the small-output convolution
(csrc/skp_conv_out.hip) against fp64, their gates and C entries; the fused VAE decoder and the DDIM sampling loop of
`ptp_utils.text2image_ldm_stable` against an fp64 copy of the same modules on the host, with the routes they take.

Kernel tolerances are those of the sibling convolution tests (tests/test_conv_s2w_gpu.py).  Module tolerances are derived in the
test: the error of the EAGER fp32 modules (same weights, no fused kernels) on the GPU against the fp64 result, times 4 -- the margin
covers the Winograd kernels' larger rounding, as tests/_tol.py does with 2x for whole steps."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

F = torch.nn.functional


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def _ref64(x, w, b):
    return F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), None if b is None else b.double(), padding=1)


def _case(B, ci, co, H, W, bias, seed=31):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    b = torch.randn(co, generator=g) if bias else None
    return x, w, b


def _run_up2(ops, x, w, b, route):
    """conv3x3_up2 with the ledger checked: `route` is the `upsample_conv` route the call must note."""
    from stablekeypoints_amd import routes
    before = routes.snapshot()
    with torch.no_grad():
        y = ops.conv3x3_up2(x, w, b)
    d = routes.delta(before)
    assert d.get(("upsample_conv", route), 0) == 1 and sum(c for (s, _), c in d.items() if s == "upsample_conv") == 1, d
    return y


# one tile, one channel block; Ci no multiple of 32, non-square, ragged last tile in both directions; odd batch, three channel
# groups; more tiles than a chip holds workgroups at once (17 x 9 tiles)
@pytest.mark.parametrize("B,ci,co,H,W,bias", [(1, 16, 32, 8, 8, True), (2, 48, 64, 12, 20, False), (3, 32, 96, 16, 40, True),
                                              (1, 16, 32, 128, 136, True)])
def test_up2_vs_fp64_and_deterministic(ops, tune, B, ci, co, H, W, bias):
    x, w, b = _case(B, ci, co, H, W, bias)
    ref = _ref64(x, w, b)
    xg, wg, bg = x.cuda(), w.cuda(), None if b is None else b.cuda()
    tune("conv_up2", 1)
    assert ops.N.lib().skp_conv3x3_up2_ok(B, ci, co, H, W) == 1
    y = _run_up2(ops, xg, wg, bg, "up2_poly")
    y2 = _run_up2(ops, xg, wg, bg, "up2_poly")
    assert y.shape == ref.shape
    err = ((y.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    print(f"up2 {B}x{ci}->{co} @{H}x{W}: max|y - y64| / max|y64| = {err:.3e}")
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())
    assert torch.equal(y, y2)                                   # no K split, no atomics: the same bits


def test_up2_corner_and_edge_pixels(ops, tune):
    """One non-zero pixel at each corner, on each edge and inside (on both sides of a tile seam), distinct values in distinct
    channels: the phase a tap belongs to, the tile it lands in and the zero border."""
    B, ci, co, H, W = 2, 16, 32, 12, 20
    x = torch.zeros(B, ci, H, W)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 9), (H - 1, 10), (5, 0), (6, W - 1), (7, 15), (8, 16), (3, 3)]
    for n, (r, c) in enumerate(spots):
        x[n % B, n % ci, r, c] = 1.0 + 0.25 * n
    g = torch.Generator().manual_seed(3)
    w = torch.randn(co, ci, 3, 3, generator=g)
    b = torch.randn(co, generator=g)
    ref = _ref64(x, w, b)
    tune("conv_up2", 1)
    y = _run_up2(ops, x.cuda(), w.cuda(), b.cuda(), "up2_poly")
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=2e-5 * ref.abs().max().item())


def test_up2_gate_and_c_abi(ops, tune):
    """The gate refuses what the kernel cannot run even when forced, and everything when switched off; a refused shape takes
    interpolate + the stride-1 route and still matches fp64; the C entries answer bad arguments with an error code, before any
    launch."""
    lib = ops.N.lib()
    tune("conv_up2", 1)
    assert lib.skp_conv3x3_up2_ok(1, 32, 64, 8, 8) == 1
    assert lib.skp_conv3x3_up2_ok(1, 24, 64, 8, 8) == 0 and lib.skp_conv3x3_up2_ok(1, 32, 48, 8, 8) == 0
    tune("conv_up2", 2)
    assert lib.skp_conv3x3_up2_ok(1, 32, 64, 8, 8) == 0
    x, w, b = _case(2, 32, 64, 16, 16, True, seed=5)
    y = _run_up2(ops, x.cuda(), w.cuda(), b.cuda(), "interp_wino")
    ref = _ref64(x, w, b)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=6e-5 * ref.abs().max().item())     # F(4x4,3x3): test_kernels_gpu's bound
    tune("conv_up2", 1)
    x, w, b = _case(2, 32, 48, 16, 16, True, seed=6)            # Co = 48: refused although forced
    y = _run_up2(ops, x.cuda(), w.cuda(), b.cuda(), "interp_wino")
    ref = _ref64(x, w, b)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=6e-5 * ref.abs().max().item())
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    BAD, RANGE = -1, -2
    assert lib.skp_conv3x3_up2_filter_f32(None, p, 32, 16, None) == BAD
    assert lib.skp_conv3x3_up2_filter_f32(p, None, 32, 16, None) == BAD
    assert lib.skp_conv3x3_up2_filter_f32(p, p, 0, 16, None) == BAD
    assert lib.skp_conv3x3_up2_filter_f32(p, p, 32, 24, None) == RANGE
    assert lib.skp_conv3x3_up2_filter_f32(p, p, 8192, 8192, None) == RANGE            # U past 2 GiB
    assert lib.skp_conv3x3_up2_f32(None, p, None, p, 1, 16, 32, 8, 8, None) == BAD
    assert lib.skp_conv3x3_up2_f32(p, None, None, p, 1, 16, 32, 8, 8, None) == BAD
    assert lib.skp_conv3x3_up2_f32(p, p, None, None, 1, 16, 32, 8, 8, None) == BAD
    assert lib.skp_conv3x3_up2_f32(p, p, None, p, 0, 16, 32, 8, 8, None) == BAD
    assert lib.skp_conv3x3_up2_f32(p, p, None, p, 1, 24, 32, 8, 8, None) == RANGE
    assert lib.skp_conv3x3_up2_f32(p, p, None, p, 1, 16, 48, 8, 8, None) == RANGE
    assert lib.skp_conv3x3_up2_f32(p, p, None, p, 64, 128, 128, 256, 256, None) == RANGE   # y past 2 GiB
    assert lib.skp_conv3x3_small_out_f32(None, p, None, p, 1, 16, 3, 8, 8, 0, None) == BAD
    assert lib.skp_conv3x3_small_out_f32(p, p, None, p, 1, 24, 3, 8, 8, 0, None) == RANGE
    assert lib.skp_conv3x3_small_out_f32(p, p, None, p, 1, 16, 5, 8, 8, 0, None) == RANGE
    assert lib.skp_conv3x3_small_out_f32(p, p, None, p, 1, 16, 3, 8, 7, 0, None) == RANGE
    assert lib.skp_axpby_f32(p, None, p, 4, 1.0, 1.0, None) == BAD
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(64))              # nothing was launched


@pytest.mark.parametrize("B,ci,co,H,W", [(1, 32, 3, 16, 24), (2, 128, 3, 64, 64), (1, 16, 4, 8, 8)])
def test_small_out_conv_vs_fp64_with_and_without_image_epilogue(ops, B, ci, co, H, W):
    from stablekeypoints_amd import routes
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5) * 2.0      # outputs on both sides of the clamp
    b = torch.randn(co, generator=g) * 0.5
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref_img = (ref / 2 + 0.5).clamp(0, 1)
    before = routes.snapshot()
    y = ops.conv3x3_small_out(x.cuda(), w.cuda(), b.cuda())
    yi = ops.conv3x3_small_out(x.cuda(), w.cuda(), b.cuda(), image=True)
    assert routes.delta(before) == {("conv_out", "small_out"): 2}
    atol = 2e-5 * ref.abs().max().item()
    torch.testing.assert_close(y.cpu().double(), ref, rtol=1e-4, atol=atol)
    torch.testing.assert_close(yi.cpu().double(), ref_img, rtol=1e-4, atol=atol + 1e-6)
    assert float(yi.min()) >= 0.0 and float(yi.max()) <= 1.0 and float(yi.min()) == 0.0 and float(yi.max()) == 1.0
    u8 = (yi.cpu() * 255).numpy().astype("uint8").astype("int32")
    u8_ref = (ref_img * 255).numpy().astype("uint8").astype("int32")
    assert abs(u8 - u8_ref).max() <= 1
    y_nobias = ops.conv3x3_small_out(x.cuda(), w.cuda(), None)
    torch.testing.assert_close(y_nobias.cpu().double(), ref - b.double()[None, :, None, None], rtol=1e-4, atol=atol)


# ---------------------------------------------------------------------------------------------------------------------------
# module level: the reduced-width tree, 64^2 images (8^2 latents)
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 4


@pytest.fixture(scope="module")
def trees():
    """(fused pipeline on the GPU, the same modules eager on the GPU, their fp64 copy on the host, embedding, latent).  All three
    hold the same seeded weights; the references are computed once here and only read by the tests."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True)
    sched_kw = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    plain = StableDiffusionPipeline.from_pretrained("tiny", scheduler=DDIMScheduler(**sched_kw), with_decoder=True)
    for k, v in ldm.vae.state_dict().items():
        assert torch.equal(v.cpu(), plain.vae.state_dict()[k]), k
    cpu64 = copy.deepcopy(plain)
    cpu64.unet.double(); cpu64.vae.double()
    eager = plain.to("cuda")
    g = torch.Generator().manual_seed(11)
    emb = torch.randn(1, 16, 768, generator=g)
    latent = torch.randn(1, 4, 8, 8, generator=g)
    z = torch.randn(2, 4, 8, 8, generator=g)

    def loop(pipe, dtype, device):
        """The sampling loop on a pipeline's own modules: UNet, scheduler step (closed form), decode, [0, 1] map."""
        pipe.scheduler.set_timesteps(STEPS)
        lat, e = latent.to(device=device, dtype=dtype), emb.to(device=device, dtype=dtype)
        acp = pipe.scheduler.alphas_cumprod.double()
        for t in pipe.scheduler.timesteps:
            eps = pipe.unet(lat, t, e)["sample"]
            t_, p_ = int(t), int(t) - 1000 // STEPS
            a_t, a_p = float(acp[t_]), float(acp[p_]) if p_ >= 0 else float(acp[0])
            x0 = (lat - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
            lat = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps
        return (pipe.vae.decode(lat / 0.18215)["sample"] / 2 + 0.5).clamp(0, 1)

    with torch.no_grad():
        ref = dict(dec64=cpu64.vae.decode(z.double())["sample"], dec_eager=eager.vae.decode(z.cuda())["sample"].cpu().double(),
                   img64=loop(cpu64, torch.float64, "cpu"), img_eager=loop(eager, torch.float32, "cuda").cpu().double())
    return dict(ldm=ldm, controllers=controllers, emb=emb, latent=latent, z=z, ref=ref, ptp=ptp_utils)


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def test_decoder_vs_fp64_and_routes(trees, tune):
    """`vae.decode` fused on the GPU against the fp64 host copy of the same modules, tolerance 4x the eager fp32 modules' own error.
    Measured on the MI355X (profiles/generate_decoder.md): see the numbers recorded there.
    The same decode under `routes.strict`: three up-samplers on the polyphase kernel, conv_out on the small-output kernel."""
    from stablekeypoints_amd import routes
    ldm, z, ref = trees["ldm"], trees["z"], trees["ref"]
    e_eager = _rel(ref["dec_eager"], ref["dec64"])
    tune("conv_up2", 1)                                         # the measured gate is about full-width shapes; these are 32 channels
    with torch.no_grad():
        before = routes.snapshot()
        with routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
            y = ldm.vae.decode(z.cuda())["sample"]
        d = routes.delta(before)
        y_img = ldm.vae.decode(z.cuda(), to_image=True)["sample"]
    e_fused = _rel(y.cpu().double(), ref["dec64"])
    print(f"decoder tiny [2,4,8,8]: eager fp32 vs fp64 {e_eager:.3e}, fused vs fp64 {e_fused:.3e} (bound {4 * e_eager:.3e})")
    print(routes.table(d))
    assert y.shape == (2, 3, 64, 64)
    assert e_fused <= 4 * e_eager
    assert d.get(("upsample_conv", "up2_poly"), 0) == 3 and d.get(("conv_out", "small_out"), 0) == 1
    assert ("conv_out", "lib") not in d and ("upsample_conv", "interp_wino") not in d and ("conv3x3", "lib") not in d
    assert d.get(("conv_in", "small"), 0) == 1 and d.get(("vae.attention", "lib_core"), 0) == 1
    torch.testing.assert_close(y_img, (y / 2 + 0.5).clamp(0, 1), rtol=0, atol=1e-6)
    # with the library's own gate the result is the same up to rounding, whichever route the up-samplers take
    tune("conv_up2", 0)
    with torch.no_grad():
        y0 = ldm.vae.decode(z.cuda())["sample"]
    assert _rel(y0.cpu().double(), ref["dec64"]) <= 4 * e_eager


def test_plain_unet_forward_notes_no_upsample_conv(trees):
    """Outside the sampling loop the UNet's up-samplers keep their present routes: a full forward notes nothing at `upsample_conv`;
    inside `ops.up2_in_unet()` the same forward notes its three up-samplers there."""
    from stablekeypoints_amd import ops, routes
    ldm, ptp = trees["ldm"], trees["ptp"]
    lat = trees["latent"].cuda().repeat(2, 1, 1, 1)

    def forward():
        before = routes.snapshot()
        with torch.no_grad():
            ptp.find_pred_noise(ldm, None, trees["emb"].cuda(), device="cuda", noise=torch.zeros_like(lat), early_exit=False,
                                controllers=trees["controllers"], latents=lat)
        for c in trees["controllers"].values():
            c.reset()
        return routes.delta(before)
    d = forward()
    assert not [k for k in d if k[0] == "upsample_conv"], d
    with ops.up2_in_unet():
        d2 = forward()
    assert sum(c for (s, _), c in d2.items() if s == "upsample_conv") == 3, d2
    assert not ops.up2_in_unet_enabled()


def test_sampling_vs_fp64_loop(trees, tune):
    """`text2image_ldm_stable`, 4 steps at 64^2 from a given latent, against the same loop on the fp64 host copy; tolerance 4x the
    eager fp32 loop's own error (both recorded in profiles/generate_decoder.md).  uint8 output shape; equal seeds give equal images."""
    ldm, ptp, ref = trees["ldm"], trees["ptp"], trees["ref"]
    ctrl = next(iter(trees["controllers"].values()))
    e_eager = _rel(ref["img_eager"], ref["img64"])
    kw = dict(num_inference_steps=STEPS, height=64, width=64)
    for force in (1, 0):                                        # the up-samplers on the polyphase kernel / on the library's own gate
        tune("conv_up2", force)
        img, lat0 = ptp.text2image_ldm_stable(ldm, trees["emb"], ctrl, latent=trees["latent"], output_type="float", **kw)
        assert img.shape == (1, 3, 64, 64) and img.is_cuda and torch.equal(lat0, trees["latent"])
        e_fused = _rel(img.cpu().double(), ref["img64"])
        print(f"sampling tiny 4 steps 64^2 (conv_up2={force}): eager fp32 loop vs fp64 {e_eager:.3e}, fused vs fp64 {e_fused:.3e} "
              f"(bound {4 * e_eager:.3e})")
        assert e_fused <= 4 * e_eager
    assert not ctrl.step_store["attn"]                          # the hooked store is left empty
    assert int(ldm.scheduler.timesteps[0]) == 980               # the optimisation path's 50-step table is back
    a, _ = ptp.text2image_ldm_stable(ldm, trees["emb"], ctrl, generator=torch.Generator().manual_seed(4), **kw)
    b, _ = ptp.text2image_ldm_stable(ldm, trees["emb"], ctrl, generator=torch.Generator().manual_seed(4), **kw)
    assert a.shape == (1, 64, 64, 3) and str(a.dtype) == "uint8"
    assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))
