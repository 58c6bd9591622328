"""CPU tests of the image-sampling path: the filter fold of the up-sampling convolution, the DDIM step, the decoder's module tree
and its separation from the encoder / UNet weights, checkpoint loading with and without the decoder, and the host route of
`ptp_utils.text2image_ldm_stable`."""
import pytest
import torch

F = torch.nn.functional

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def test_up2_fold_filter_matches_interpolate_conv_fp64():
    """Four 2x2 convolutions of the low-resolution input with the folded phase filters, interleaved, equal
    conv2d(interpolate(x, 2x, nearest), w, padding=1) in fp64."""
    from stablekeypoints_amd import ops
    B, ci, co, H, W = 2, 48, 32, 5, 7
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) / (3 * ci ** 0.5)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    Ff = ops.up2_fold_filter(w)
    assert Ff.shape == (2, 2, co, ci, 2, 2) and Ff.dtype == torch.float64
    xp = F.pad(x, (1, 1, 1, 1))                                  # window (i + a - 1 + dr, j + c - 1 + dc): out of range = 0
    y = torch.empty_like(ref)
    for a in range(2):
        for c in range(2):
            o = F.conv2d(xp, Ff[a, c], b)                        # [B, co, H + 1, W + 1]; phase (a, c) of pixel (i, j) sits at (i + a, j + c)
            y[:, :, a::2, c::2] = o[:, :, a:a + H, c:c + W]
    assert (y - ref).abs().max().item() <= 1e-12
    # the fold keeps the filter's mass: every phase sums the same nine taps
    torch.testing.assert_close(Ff.sum(dim=(-1, -2)), w.sum(dim=(-1, -2))[None, None].expand(2, 2, -1, -1), rtol=0, atol=1e-13)


def _closed_form(acp, t, n_steps, x, eps, final, clip):
    prev = t - 1000 // n_steps
    a_t = acp[t]
    a_p = acp[prev] if prev >= 0 else final
    x0 = (x - (1 - a_t).sqrt() * eps) / a_t.sqrt()
    if clip:
        x0 = x0.clamp(-1, 1)
    return a_p.sqrt() * x0 + (1 - a_p).sqrt() * eps


@pytest.mark.parametrize("n_steps", [50, 4])
@pytest.mark.parametrize("alpha_to_one", [True, False])
@pytest.mark.parametrize("clip", [False, True])
def test_ddim_step_matches_closed_form(n_steps, alpha_to_one, clip):
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    s = DDIMScheduler(clip_sample=clip, set_alpha_to_one=alpha_to_one, **SD)
    s.set_timesteps(n_steps)
    assert s.clip_sample == clip and s.set_alpha_to_one == alpha_to_one
    acp = s.alphas_cumprod.double()
    final = torch.tensor(1.0, dtype=torch.float64) if alpha_to_one else acp[0]
    g = torch.Generator().manual_seed(n_steps)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    eps = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    ts = [int(t) for t in s.timesteps]
    assert ts[-1] == 0 and ts[0] == 1000 - 1000 // n_steps
    for t in (ts[0], ts[len(ts) // 2], ts[-1]):                  # the last step has prev_t < 0
        want = _closed_form(acp, t, n_steps, x, eps, final, clip)
        got64 = s.step(eps, torch.tensor(t), x)["prev_sample"]
        assert got64.dtype == torch.float64
        torch.testing.assert_close(got64, want, rtol=1e-12, atol=1e-12)
        got32 = s.step(eps.float(), t, x.float())["prev_sample"]
        assert got32.dtype == torch.float32
        assert ((got32.double() - want).abs().max() / want.abs().max()).item() <= 1e-6


def test_ddim_last_step_returns_x0_of_add_noise():
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    s = DDIMScheduler(clip_sample=False, set_alpha_to_one=True, **SD)
    s.set_timesteps(50)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)
    eps = torch.randn(1, 4, 8, 8, generator=g, dtype=torch.float64)
    t = s.timesteps[-1]
    x_t = s.add_noise(x0, eps, t)
    # (add_noise takes its two square roots in fp32, the step in fp64: 6e-8 relative apart)
    torch.testing.assert_close(s.step(eps, t, x_t)["prev_sample"], x0, rtol=1e-6, atol=1e-6)
    # the step reads nothing back from a device: the timestep table lives on the host
    assert s.timesteps.device.type == "cpu" and s.alphas_cumprod.device.type == "cpu"


DECODER_KEYS_PER_RESNET = ("norm1", "conv1", "norm2", "conv2")


def _expected_decoder_modules(boc):
    rev = list(reversed(boc))
    mods = ["decoder.conv_in", "decoder.conv_norm_out", "decoder.conv_out", "post_quant_conv"]
    mods += [f"decoder.mid_block.resnets.{i}.{m}" for i in range(2) for m in DECODER_KEYS_PER_RESNET]
    mods += [f"decoder.mid_block.attentions.0.{m}" for m in ("group_norm", "query", "key", "value", "proj_attn")]
    ch = rev[0]
    for b, oc in enumerate(rev):
        for r in range(3):
            mods += [f"decoder.up_blocks.{b}.resnets.{r}.{m}" for m in DECODER_KEYS_PER_RESNET]
            if r == 0 and ch != oc:
                mods.append(f"decoder.up_blocks.{b}.resnets.{r}.conv_shortcut")
        if b != len(rev) - 1:
            mods.append(f"decoder.up_blocks.{b}.upsamplers.0.conv")
        ch = oc
    return sorted(f"{m}.{p}" for m in mods for p in ("weight", "bias"))


def test_decoder_tree_has_the_diffusers_keys():
    from stablekeypoints_amd.ldm.vae import AutoencoderKL
    with torch.device("meta"):
        vae = AutoencoderKL()
        n_enc = len(vae.state_dict())
        vae.add_decoder(0)
    keys = dict(vae.state_dict())
    dec = sorted(k for k in keys if k.startswith(("decoder.", "post_quant_conv.")))
    assert dec == _expected_decoder_modules((128, 256, 512, 512))
    assert len([k for k in dec if k.startswith("decoder.")]) == 138 and len(keys) == n_enc + 140
    assert "decoder.up_blocks.2.resnets.0.conv_shortcut.weight" in keys and "decoder.up_blocks.3.resnets.0.conv_shortcut.weight" in keys
    assert tuple(keys["decoder.conv_in.weight"].shape) == (512, 4, 3, 3)
    assert tuple(keys["decoder.up_blocks.2.resnets.0.conv1.weight"].shape) == (256, 512, 3, 3)
    assert tuple(keys["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"].shape) == (128, 256, 1, 1)
    assert tuple(keys["decoder.up_blocks.2.upsamplers.0.conv.weight"].shape) == (256, 256, 3, 3)
    assert tuple(keys["decoder.conv_out.weight"].shape) == (3, 128, 3, 3) and tuple(keys["post_quant_conv.weight"].shape) == (4, 4, 1, 1)
    assert vae.decoder.conv_norm_out.eps == 1e-6 and vae.decoder.up_blocks[0].resnets[0].norm1.eps == 1e-6


def test_weights_without_decoder_are_unchanged_by_it():
    """The decoder is drawn after everything else from a generator of its own: the UNet's and the encoder's tensors are the same
    with and without it, a model without it has no decoder key, and the global generator is where it was."""
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    a = StableDiffusionPipeline.from_pretrained("tiny")
    b = StableDiffusionPipeline.from_pretrained("tiny", with_decoder=True)
    assert torch.equal(torch.random.get_rng_state(), before)
    assert not a.vae.has_decoder and b.vae.has_decoder
    for ma, mb in ((a.unet, b.unet), (a.vae, b.vae)):
        sa, sb = ma.state_dict(), mb.state_dict()
        assert not [k for k in sa if k.startswith(("decoder.", "post_quant_conv."))]
        assert set(sa) <= set(sb) and all(k.startswith(("decoder.", "post_quant_conv.")) for k in set(sb) - set(sa))
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    assert sorted(k for k in b.vae.state_dict() if k.startswith(("decoder.", "post_quant_conv."))) == _expected_decoder_modules((32, 32, 32, 32))
    # same seed, same decoder; the decoder does not repeat the encoder's draws
    c = StableDiffusionPipeline.from_pretrained("tiny", with_decoder=True)
    assert torch.equal(b.vae.decoder.conv_in.weight, c.vae.decoder.conv_in.weight)
    assert not torch.equal(b.vae.decoder.mid_block.resnets[0].conv1.weight, b.vae.encoder.mid_block.resnets[0].conv1.weight)
    with pytest.raises(RuntimeError, match="decoder=True"):
        a.vae.decode(torch.zeros(1, 4, 8, 8))
    with torch.no_grad():
        y = b.vae.decode(torch.zeros(1, 4, 8, 8))["sample"]
        yi = b.vae.decode(torch.zeros(1, 4, 8, 8), to_image=True)["sample"]
    assert y.shape == (1, 3, 64, 64) and torch.equal(yi, (y / 2 + 0.5).clamp(0, 1))


def test_checkpoint_decoder_keys_tolerated_or_checked(tmp_path):
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.optimize_token import load_ldm
    unet, vae = StableDiffusionPipeline.build("tiny", seed=7, with_decoder=True)
    d = tmp_path / "tiny-ckpt"
    d.mkdir()
    torch.save(unet.state_dict(), str(d / "unet.pt"))
    torch.save(vae.state_dict(), str(d / "vae.pt"))
    import stablekeypoints_amd.ldm.pipeline as P
    orig = P.guess_arch
    P.guess_arch = lambda name: "tiny"
    try:
        ldm, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32)                 # decoder keys: tolerated leftovers
        assert not ldm.vae.has_decoder and torch.equal(ldm.vae.encoder.conv_in.weight, vae.encoder.conv_in.weight)
        ldm, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32, decoder=True)   # ... loaded and checked
        assert ldm.vae.has_decoder and not ldm.synthetic_weights
        for k, v in vae.state_dict().items():
            assert torch.equal(ldm.vae.state_dict()[k], v), k
        assert not any(p.requires_grad for p in ldm.vae.parameters())
        sd = vae.state_dict(); sd.pop("decoder.up_blocks.1.upsamplers.0.conv.bias")
        torch.save(sd, str(d / "vae.pt"))
        with pytest.raises(RuntimeError, match="1 missing"):
            load_ldm("cpu", str(d), feature_upsample_res=32, decoder=True)
        load_ldm("cpu", str(d), feature_upsample_res=32)                             # still fine without the decoder
    finally:
        P.guess_arch = orig


def test_text2image_on_the_host_route():
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.optimize_token import load_ldm
    for name in ("diffusion_step", "latent2image", "init_latent", "latent_step", "text2image_ldm_stable"):
        assert callable(getattr(ptp_utils, name)), name
    ldm, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True)
    ctrl = next(iter(controllers.values()))
    emb = torch.randn(1, 16, 768, generator=torch.Generator().manual_seed(3))
    kw = dict(num_inference_steps=3, height=64, width=64)
    before = routes.snapshot()
    img, lat = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=torch.Generator().manual_seed(5), **kw)
    assert not [k for k in routes.delta(before) if k[0] == "upsample_conv"]           # host tensors: the modules' own forward
    assert img.shape == (1, 64, 64, 3) and str(img.dtype) == "uint8" and lat.shape == (1, 4, 8, 8)
    assert torch.equal(lat, torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(5)))       # the reference's draw
    img2, _ = ptp_utils.text2image_ldm_stable(ldm, emb, None, generator=torch.Generator().manual_seed(5), **kw)
    img3, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, **kw)
    assert (img == img2).all() and (img == img3).all()
    other, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=torch.Generator().manual_seed(6), **kw)
    assert (img != other).any()
    fl, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, output_type="float", **kw)
    assert fl.shape == (1, 3, 64, 64) and fl.dtype == torch.float32 and 0.0 <= float(fl.min()) and float(fl.max()) <= 1.0
    assert ((fl.permute(0, 2, 3, 1).numpy() * 255).astype("uint8") == img).all()
    assert not ctrl.step_store["attn"] and int(ldm.scheduler.timesteps[0]) == 980     # store empty, the 50-step table restored
    # the pieces, by the reference's signatures
    lat_a, lats = ptp_utils.init_latent(None, ldm, 64, 64, torch.Generator().manual_seed(5))
    assert torch.equal(lat_a, lat) and lats.shape == (1, 4, 8, 8)
    t = ldm.scheduler.timesteps[0]
    with torch.no_grad():
        eps = ptp_utils.diffusion_step(ldm, lats, emb, t)
        nxt = ptp_utils.latent_step(ldm, ctrl, lats, [None, emb], t, 7.5)
    torch.testing.assert_close(nxt, ldm.scheduler.step(eps, t, lats)["prev_sample"])
    ctrl.reset()
    with pytest.raises(NotImplementedError):
        ptp_utils.latent_step(ldm, ctrl, lats, [None, emb], t, 7.5, low_resource=False)
    assert ptp_utils.latent2image(ldm.vae, lats).shape == (1, 64, 64, 3)
    plain, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=32)
    with pytest.raises(RuntimeError, match="decoder=True"):
        ptp_utils.text2image_ldm_stable(plain, emb, None, **kw)
