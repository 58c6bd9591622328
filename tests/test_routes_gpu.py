"""The route ledger on the MI355X: the routes of the three supported architectures are pinned, a forced gate regression is seen,
replayed graphs keep count, and `routes="strict"` raises at the gate (stablekeypoints_amd/routes.py)."""
import pytest
import torch
from _tol import GRAD_TOL

from oracle import ref_path as R

pytestmark = pytest.mark.gpu

# the sites a 3x3 Conv2d module's forward can note (a Downsample2D that runs its own forward runs its own 3x3 Conv2d: one note)
CONV_SITES = ("conv3x3", "conv_in", "conv_out", "conv3x3_s2", "downsample.untiled")


def _site_total(counts, sites):
    return sum(c for (s, _), c in counts.items() if s in sites)


def _count(counts, site, route):
    return counts.get((site, route), 0)


def _conv3x3_modules(*trees):
    return sum(1 for t in trees for m in t.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3))


def _sd15_inputs(n_img):
    """The inputs of tests/test_round4_gpu.py::test_sd15_config2_shape_step_vs_oracle (BASELINE config 2's launch shape)."""
    g = torch.Generator().manual_seed(7)
    images4 = torch.rand(4, 3, 512, 512, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g) * 5.0
    noise4 = torch.randn(8, 4, 64, 64, generator=g)
    thetas4 = torch.cat([R.affine_matrix(a, s, tr) for a, s, tr in
                         ((9.0, 0.9, (0.1, -0.15)), (-12.0, 0.85, (-0.2, 0.05)), (4.0, 0.97, (0.0, 0.22)), (-7.0, 0.8, (0.18, 0.1)))])
    return images4[:n_img], ctx, torch.cat([noise4[:n_img], noise4[4:4 + n_img]]), thetas4[:n_img]


@pytest.fixture(scope="module")
def sd15():
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cuda", "sd15", feature_upsample_res=128, init_on_device=True)
    return ldm, controllers


def test_pinned_routes_sd15_group_step(sd15):
    """Full-width SD-1.5 at 512^2, 4 images x 2 views, T = 77, R = 128: forward + backward of one `group_step` takes HIP routes
    only, bar the documented library routes -- and takes the routes a gate regression would lose.

    Convolution count: every 3 x 3 Conv2d of the UNet and of the VAE encoder is reached exactly once by one FULL forward (the
    step itself stops the UNet after the last stored map, so it reaches a prefix only), and each notes exactly one of the sites
    `conv3x3`, `conv_in`, `conv_out`, `conv3x3_s2`, or -- the 16^2 -> 8^2 Downsample2D, below the stride-2 kernel's tile, on its own
    forward -- `downsample.untiled` (the VAE's conv_out + quant_conv run as one composed 3 x 3 convolution, noted
    as `conv3x3`).  So the notes of those sites over one VAE encode + one full UNet forward equal the number of 3 x 3 Conv2d
    modules in the two trees; the step's own count is that of the encode plus a prefix of the UNet's.  The full forward runs at 2
    rows, the smallest batch the product launches (one image and its affine copy); a single row is no product shape, and the
    640 -> 1280 convolution at 16^2 has too few tiles for the Winograd kernels there."""
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    from stablekeypoints_amd.optimize import default_args, group_step
    ldm, controllers = sd15
    dev, controller = next(iter(controllers.items()))
    n_img = 4
    images, ctx, noise, thetas = _sd15_inputs(n_img)
    args = default_args(num_tokens=77, feature_upsample_res=128, furthest_point_num_samples=25, top_k=10, batch_size=n_img)
    c_gpu = ctx.clone().cuda().requires_grad_(True)
    routes.reset()
    with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
        group_step(ldm, images, c_gpu, args, controller, RandomAffineWithInverse(), denom=n_img, noise=noise.cuda(), thetas=thetas)
        torch.cuda.synchronize()
    step = routes.snapshot()
    print(routes.table(step))
    assert torch.isfinite(c_gpu.grad).all()
    # the >= 1024-key self-attention layers (64^2 and 32^2) run the split-bf16 flash kernels, forward and backward
    assert _count(step, "flash.fwd", "flash_split") > 0 and _count(step, "flash.bwd", "flash_split") > 0
    assert _count(step, "conv3x3", "wino4_c128") > 0 and _count(step, "conv3x3", "wino4_raw") > 0
    assert _count(step, "conv3x3.bwd_data", "wino4_c128") > 0 and _count(step, "conv3x3.bwd_data", "wino4_raw") > 0
    assert _count(step, "conv3x3", "lib") == 0 and _count(step, "conv3x3.bwd_data", "lib") == 0
    assert _count(step, "downsample", "eager") == 0 and _count(step, "downsample", "s2_direct") > 0
    assert _count(step, "resnet", "eager") == 0 and _count(step, "resnet", "fused") > 0
    assert _count(step, "transformer2d", "eager") == 0 and _count(step, "transformer_block", "eager") == 0
    assert _count(step, "group_norm", "gn_fold") > 0                        # the VAE's 128- and 256-channel levels
    assert _count(step, "vae.tail", "composed") == 1 and _count(step, "vae.attention", "lib_core") == 1
    assert _count(step, "map.fwd", "map_fused") == 1 and _count(step, "map.bwd", "map_col") == 1
    assert _count(step, "attn.cross", "ca_token_split") + _count(step, "attn.cross", "ca_plain") > 0
    assert {r for (s, r) in step if s in ("attn.cross", "attn.self")} <= {"ca_token_split", "ca_plain", "fused_qkv", "plain"}
    # one VAE encode + one FULL UNet forward: every 3 x 3 convolution module notes once
    n_vae, n_unet = _conv3x3_modules(ldm.vae), _conv3x3_modules(ldm.unet)
    with torch.no_grad():
        routes.reset()
        lat = ptp_utils.image2latent(ldm, images[:2].cuda(), dev)
        enc = routes.snapshot()
        routes.reset()
        with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
            ptp_utils.find_pred_noise(ldm, None, ctx.cuda(), device=dev, noise=noise[:2].cuda(), early_exit=False,
                                      controllers=controllers, latents=lat)
        full = routes.snapshot()
        controller.reset()
    print("3x3 Conv2d modules: vae", n_vae, "unet", n_unet, "| noted: encode", _site_total(enc, CONV_SITES), "full unet forward",
          _site_total(full, CONV_SITES))
    assert _site_total(enc, CONV_SITES) == n_vae
    assert _site_total(full, CONV_SITES) == n_unet
    assert _count(full, "conv_out", "lib") == 1 and _count(full, "conv3x3", "lib") == 0        # 320 -> 4: the documented odd shape
    # the step: the encode's convolutions and a prefix of the UNet's forward; its backward reaches no more than the forward did
    fwd_step = _site_total(step, CONV_SITES)
    assert n_vae < fwd_step <= n_vae + n_unet
    assert 0 < _site_total(step, ("conv3x3.bwd_data",)) <= fwd_step - n_vae


def test_pinned_routes_sd21_sdxl_one_forward():
    """The full-width one-forward shapes of tests/test_round2_gpu.py::test_sd21_sdxl_full_width_trees_one_forward (SD-2.1 at 768^2,
    SDXL at 1024^2, one image, T = 77): HIP routes only, bar the documented library routes."""
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd._maps import collect_maps_batched
    from stablekeypoints_amd.optimize_token import load_ldm
    for arch, size, width in (("sd21", 768, 1024), ("sdxl", 1024, 2048)):
        ldm, controllers, _ = load_ldm("cuda", arch, feature_upsample_res=128, init_on_device=True)
        dev, controller = next(iter(controllers.items()))
        g = torch.Generator().manual_seed(1)
        img = torch.rand(1, 3, size, size, generator=g).cuda()
        ctx = torch.randn(1, 77, width, generator=g).cuda().requires_grad_(True)
        routes.reset()
        with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
            ptp_utils.find_pred_noise(ldm, img, ctx, device=dev, early_exit=True, controllers=controllers)
            M = collect_maps_batched(controller)
            torch.cuda.synchronize()
        snap = routes.snapshot()
        print(arch)
        print(routes.table(snap))
        assert M.shape == (1, 77, 128, 128)
        assert _count(snap, "resnet", "fused") > 0 and _count(snap, "transformer2d", "fused") > 0
        assert _count(snap, "conv3x3", "lib") == 0 and _count(snap, "map.fwd", "map_fused") == 1
        assert _count(snap, "flash.fwd", "flash_f32") + _count(snap, "flash.fwd", "flash_split") > 0     # 64-wide heads
        del ldm, controllers, controller, M
        torch.cuda.empty_cache()


def test_forced_gate_regressions_are_seen(sd15, monkeypatch, tune):
    """Three ways a gate can regress without changing a value, each seen by the ledger (SD-1.5, 512^2, one image x 2 views,
    forward without autograd):
      * `ops.CONV3X3_MODE = "lib"`: `expect` raises naming conv3x3 / lib;
      * `skp_tune_set("gn_fold_max_cout", 1)`: the VAE encoder's folded GroupNorms all become apply passes -- `gn_fold` drops to
        zero, `gn_apply` rises by the same amount -- and the latents stay within tests/_tol.py's 3e-5 of their maximum;
      * `ops.FLASH_SPLIT = False`: the `flash_split` launches become `flash_f32` ones."""
    from stablekeypoints_amd import ops, ptp_utils, routes
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    ldm, controllers = sd15
    dev, controller = next(iter(controllers.items()))
    images, ctx, noise, thetas = _sd15_inputs(1)
    both = torch.cat([images.cuda(), RandomAffineWithInverse()(images.cuda(), theta=thetas)])

    def forward():
        routes.reset()
        with torch.no_grad():
            lat = ptp_utils.image2latent(ldm, both, dev)
            ptp_utils.find_pred_noise(ldm, None, ctx.cuda(), device=dev, noise=noise.cuda(), early_exit=True, controllers=controllers,
                                      latents=lat)
            torch.cuda.synchronize()
        controller.reset()
        return lat, routes.snapshot()

    lat0, base = forward()
    fold0, apply0 = _count(base, "group_norm", "gn_fold"), _count(base, "group_norm", "gn_apply")
    split0, f32_0 = _count(base, "flash.fwd", "flash_split"), _count(base, "flash.fwd", "flash_f32")
    assert fold0 > 0 and split0 > 0 and _count(base, "conv3x3", "lib") == 0

    with monkeypatch.context() as mp:
        mp.setattr(ops, "CONV3X3_MODE", "lib")
        with pytest.raises(routes.UnexpectedRoute) as err:
            with routes.expect(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
                forward()
        controller.reset()
    assert any(s == "conv3x3" and r == "lib" and n > 0 for s, r, n in err.value.found), err.value.found
    assert "conv3x3/lib" in str(err.value)
    # every Downsample2D was refused for the mode, not for the kernel's tile: none of them may pass as the documented untiled site
    found = {(s, r): n for s, r, n in err.value.found}
    assert found.get(("downsample", "eager"), 0) > 0 and _count(routes.snapshot(), "downsample.untiled", "eager") == 0

    tune("gn_fold_max_cout", 1)
    lat1, nofold = forward()
    tune("gn_fold_max_cout", 0)
    assert _count(nofold, "group_norm", "gn_fold") == 0
    assert _count(nofold, "group_norm", "gn_apply") == apply0 + fold0
    err_lat = ((lat1 - lat0).abs().max() / lat0.abs().max()).item()
    print(f"latents folded vs un-folded GroupNorm: max|diff| / max = {err_lat:.3e} (tol {GRAD_TOL:.1e})")
    assert err_lat <= GRAD_TOL

    with monkeypatch.context() as mp:
        mp.setattr(ops, "FLASH_SPLIT", False)
        _, f32 = forward()
    assert _count(f32, "flash.fwd", "flash_split") == 0
    assert _count(f32, "flash.fwd", "flash_f32") == f32_0 + split0


def test_replayed_graph_keeps_count():
    """`GraphedStep` on the reduced-width tree at 512^2 / R = 128, one image per group (the shape of
    tests/test_round6_gpu.py::test_graphed_step_replays_the_eager_step), warmup = 2, five calls.

    Accounting rule: the `warmup` eager calls count as the eager steps they are (E each).  The call that captures adds P, the
    one-image VAE encode that reads the latent geometry before the recording and really runs; the recording itself runs every
    gate but launches nothing, so its notes D leave the ledger again and are kept with the graph; that call's replay and every
    later replay add D.  The captured body takes the eager step's routes, D == E, hence after 2 warm-up calls, the capture and
    3 replays in all:   snapshot == 2 E + P + 3 E,   exactly."""
    from test_e2e_gpu import _setup
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    from stablekeypoints_amd.optimize import GraphedStep, group_step
    ldm, controllers, cpu, images, ctx, noise, args = _setup(R_up=128, T=16, n=2, size=512)
    del cpu
    dev, controller = next(iter(controllers.items()))
    g = torch.Generator().manual_seed(5)
    tr_a, tr_b = RandomAffineWithInverse(15, (0.8, 1.0), (0.25, 0.25)), RandomAffineWithInverse(15, (0.8, 1.0), (0.25, 0.25))
    c_e = ctx.clone().cuda().requires_grad_(True)
    c_g = ctx.clone().cuda().requires_grad_(True)
    img = torch.rand(1, 3, 512, 512, generator=g)
    nz = torch.randn(2, 4, 64, 64, generator=g).cuda()
    th = R.affine_matrix(7.0, 0.9, (0.1, -0.05))
    routes.reset()
    group_step(ldm, img, c_e, args, controller, tr_a, denom=1, noise=nz, thetas=th)
    E = routes.snapshot()
    routes.reset()
    with torch.no_grad():
        ptp_utils.image2latent(ldm, img.cuda(), dev)
    P = routes.snapshot()
    assert E and P
    graphed = GraphedStep(ldm, c_g, args, controller, tr_b, denom=1, warmup=2)
    routes.reset()
    for call in range(5):
        graphed(img, noise=nz, thetas=th)
    torch.cuda.synchronize()
    st = graphed.state[1]
    assert st != "eager" and st["graph"] is not None and st["calls"] == 2, "calls 3-5 must have been replays"
    assert st["routes"] == E, "the captured body must take the eager step's routes"
    want = {k: 5 * E.get(k, 0) + P.get(k, 0) for k in set(E) | set(P)}
    assert routes.snapshot() == want


def test_optimize_embedding_routes_strict(monkeypatch):
    """`optimize_embedding(..., routes="strict")` on the reduced-width tree, 3 steps of 8 images (16 rows: at fewer rows the
    reduced tree's 8^2 level has too few tiles for the Winograd kernels and runs on the library, which strict refuses): passes, and `routes.table()` describes the run;
    with `ops.CONV3X3_MODE = "lib"` it raises at the gate (the traceback ends in `conv3x3_auto`)."""
    import traceback
    from stablekeypoints_amd import ops, routes
    from stablekeypoints_amd.optimize import default_args, optimize_embedding
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cuda", "tiny", feature_upsample_res=128)
    args = default_args(num_tokens=16, feature_upsample_res=128, furthest_point_num_samples=8, top_k=4, batch_size=8, device="cuda",
                        num_steps=3, max_len=8, image_size=512, log_interval=0, model_type="tiny")
    with pytest.raises(ValueError, match="routes must be one of"):
        optimize_embedding(ldm, args, controllers, 1, routes="loud")
    out = optimize_embedding(ldm, args, controllers, 1, routes="strict")
    assert torch.isfinite(out).all()
    snap = routes.snapshot()
    print(routes.table(snap))
    assert _count(snap, "resnet", "fused") > 0 and _count(snap, "map.fwd", "map_fused") == 3
    assert all(routes.kind(s, r) == "hip" or (s, r) in routes.DOCUMENTED_LIBRARY_ROUTES for s, r in snap)
    monkeypatch.setattr(ops, "CONV3X3_MODE", "lib")
    with pytest.raises(routes.UnexpectedRoute) as err:
        optimize_embedding(ldm, args, controllers, 1, routes="strict")
    assert ("conv3x3", "lib", 1) in err.value.found
    assert "conv3x3_auto" in "".join(traceback.format_tb(err.value.__traceback__))
    routes.note("conv3x3", "lib")                                             # the strict rule ended with the call
