"""CPU tests of guided / batched / v-prediction image sampling: the scheduler's three prediction types and its guidance mix in fp64,
`ptp_utils.guided_latent_step` on an fp64 copy of the reduced-width tree, batches and guidance through `text2image_ldm_stable` on
the host route, and `load_ldm(prediction_type=)`."""
import copy
import json

import pytest
import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
TYPES = ("epsilon", "v_prediction", "sample")


def _coef(s, t, n_steps, alpha_to_one):
    acp = s.alphas_cumprod.double()
    prev = t - 1000 // n_steps
    a_t = acp[t]
    a_p = acp[prev] if prev >= 0 else (torch.tensor(1.0, dtype=torch.float64) if alpha_to_one else acp[0])
    return a_t.sqrt(), (1 - a_t).sqrt(), a_p.sqrt(), (1 - a_p).sqrt()


def _formula(kind, x, m, sa, sb, pa, pb, clip):
    """The update of include/skp.h, skp_ddim_step_f32, written out."""
    if kind == "epsilon":
        x0, eps = (x - sb * m) / sa, m
    elif kind == "v_prediction":
        x0, eps = sa * x - sb * m, sa * m + sb * x
    else:
        x0, eps = m, (x - sa * m) / sb
    if clip:
        x0 = x0.clamp(-1, 1)
    return pa * x0 + pb * eps


@pytest.mark.parametrize("n_steps", [4, 50])
@pytest.mark.parametrize("alpha_to_one", [True, False])
def test_prediction_types_fp64(n_steps, alpha_to_one):
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    g = torch.Generator().manual_seed(7 + n_steps)
    x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    eps = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    for clip in (False, True):
        scheds = {}
        for kind in TYPES:
            s = scheds[kind] = DDIMScheduler(clip_sample=clip, set_alpha_to_one=alpha_to_one, prediction_type=kind, **SD)
            s.set_timesteps(n_steps)
            assert s.prediction_type == kind
        ts = [int(t) for t in scheds["epsilon"].timesteps]
        assert ts[-1] == 0
        for t in (ts[0], ts[len(ts) // 2], ts[-1]):              # the last step has prev_t < 0
            sa, sb, pa, pb = _coef(scheds["epsilon"], t, n_steps, alpha_to_one)
            x_t = sa * x0 + sb * eps
            fed = {"epsilon": eps, "v_prediction": sa * eps - sb * x0, "sample": x0}
            for kind in TYPES:
                got = scheds[kind].step(fed[kind], torch.tensor(t), x_t)["prev_sample"]
                assert got.dtype == torch.float64
                if clip:
                    want = _formula(kind, x_t, fed[kind], sa, sb, pa, pb, True)
                else:
                    want = pa * x0 + pb * eps                    # the three parametrisations of one trajectory agree
                assert (got - want).abs().max().item() <= 1e-12, (kind, t, clip)


def test_unknown_prediction_type_raises():
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    with pytest.raises(ValueError):
        DDIMScheduler(prediction_type="v")
    with pytest.raises(ValueError):
        DDIMScheduler(prediction_type=None)
    assert DDIMScheduler().prediction_type == "epsilon"


@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("clip", [False, True])
def test_guidance_fp64(kind, clip):
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    s = DDIMScheduler(clip_sample=clip, set_alpha_to_one=False, prediction_type=kind, **SD)
    s.set_timesteps(4)
    g = torch.Generator().manual_seed(5)
    x, mc, mu = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(3))
    for t in s.timesteps:
        for gs in (7.5, 0, 1, -2):
            got = s.step(mc, t, x, uncond_output=mu, guidance_scale=gs)["prev_sample"]
            want = s.step(mu + gs * (mc - mu), t, x)["prev_sample"]
            assert (got - want).abs().max().item() <= 1e-12, (int(t), gs)
            two = s.step(mc, t, x, uncond_output=mu, guidance_scale=gs, copies=2)["prev_sample"]
            assert two.shape == (4, 4, 8, 8) and torch.equal(two[:2], got) and torch.equal(two[2:], got)
    got32 = s.step(mc.float(), 0, x.float(), uncond_output=mu.float(), guidance_scale=7.5)["prev_sample"]
    assert got32.dtype == torch.float32 and got32.device.type == "cpu"
    want = s.step(mc, 0, x, uncond_output=mu, guidance_scale=7.5)["prev_sample"]
    assert ((got32.double() - want).abs().max() / want.abs().max()).item() <= 1e-5
    with pytest.raises(ValueError):
        s.step(mc, 0, x, copies=3)
    with pytest.raises(TypeError):
        s.step(mc, 0, x, mu)                                    # the new arguments are keyword-only


@pytest.fixture(scope="module")
def tiny():
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True)
    return ldm, next(iter(controllers.values()))


@pytest.mark.parametrize("t_uncond", [16, 24])
def test_guided_latent_step_on_fp64_tree(tiny, t_uncond):
    """Equal token counts (one forward of 2n rows) and 16 against 24 tokens (two forwards) both equal the step built from two
    `diffusion_step` calls; in fp64 only the batch-of-two against single-row summation order differs."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    ldm, _ = tiny
    plain = StableDiffusionPipeline.from_pretrained("tiny", scheduler=DDIMScheduler(clip_sample=False, set_alpha_to_one=False, **SD))
    assert torch.equal(plain.unet.conv_in.weight, ldm.unet.conv_in.weight)                # the same seeded tree, without the hooks
    ldm64 = copy.deepcopy(plain)
    ldm64.unet.double()
    ldm64.scheduler.set_timesteps(4)
    g = torch.Generator().manual_seed(21)
    cond = torch.randn(1, 16, 768, generator=g, dtype=torch.float64)
    uncond = torch.randn(1, t_uncond, 768, generator=g, dtype=torch.float64)
    lats = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    t = ldm64.scheduler.timesteps[1]
    with torch.no_grad():
        eps_c = ptp_utils.diffusion_step(ldm64, lats, cond, t)
        eps_u = ptp_utils.diffusion_step(ldm64, lats, uncond, t)
        want = ldm64.scheduler.step(eps_c, t, lats, uncond_output=eps_u, guidance_scale=7.5)["prev_sample"]
        got = ptp_utils.guided_latent_step(ldm64, None, lats, [uncond, cond], t, 7.5)
    assert got.dtype == torch.float64 and got.shape == lats.shape
    assert (eps_c - eps_u).abs().max().item() > 1e-3             # the two contexts do predict differently
    assert (got - want).abs().max().item() <= 1e-10
    if t_uncond == 16:
        with torch.no_grad():
            two = ptp_utils.guided_latent_step(ldm64, None, torch.cat([lats, lats]), [uncond, cond], t, 7.5, doubled=True)
        assert two.shape == (4, 4, 8, 8) and torch.equal(two[:2], got) and torch.equal(two[2:], got)
    else:
        with pytest.raises(ValueError):
            ptp_utils.guided_latent_step(ldm64, None, torch.cat([lats, lats]), [uncond, cond], t, 7.5, doubled=True)


def test_text2image_batches_and_guidance_on_the_host(tiny):
    from stablekeypoints_amd import ptp_utils
    ldm, ctrl = tiny
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(1, 16, 768, generator=g)
    unc = torch.randn(1, 16, 768, generator=g)
    seeds = (5, 6, 7)

    def gens():
        return [torch.Generator().manual_seed(s) for s in seeds]
    kw = dict(num_inference_steps=4, height=64, width=64)
    img, lat = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=gens(), **kw)
    assert img.shape == (3, 64, 64, 3) and str(img.dtype) == "uint8" and lat.shape == (3, 4, 8, 8)
    for i, s in enumerate(seeds):                                # the reference's draw, image by image
        assert torch.equal(lat[i:i + 1], torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(s)))
    lat_b, lats_b = ptp_utils.init_latents(None, ldm, 64, 64, gens())
    assert torch.equal(lat_b, lat) and lats_b.shape == (3, 4, 8, 8)
    fl, lat2 = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, output_type="float", **kw)
    assert fl.shape == (3, 3, 64, 64) and torch.equal(lat2, lat)
    assert ((fl.permute(0, 2, 3, 1).numpy() * 255).astype("uint8") == img).all()
    hi, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=gens(), uncond_embedding=unc, guidance_scale=7.5, **kw)
    lo, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=gens(), uncond_embedding=unc, guidance_scale=1.0, **kw)
    hi2, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, uncond_embedding=unc, guidance_scale=7.5, **kw)
    assert hi.shape == (3, 64, 64, 3) and (hi != lo).any() and (hi == hi2).all()
    other, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, uncond_embedding=unc[:, :12], guidance_scale=7.5, **kw)
    assert other.shape == (3, 64, 64, 3) and (other != hi).any()                    # contexts of different length: two forwards
    assert not ctrl.step_store["attn"] and int(ldm.scheduler.timesteps[0]) == 980
    one, lat1 = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, generator=torch.Generator().manual_seed(5), **kw)
    assert one.shape == (1, 64, 64, 3) and lat1.shape == (1, 4, 8, 8)
    with pytest.raises(ValueError):
        ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, uncond_embedding=torch.zeros(1, 16, 32), **kw)
    with pytest.raises(ValueError):
        ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, generator=gens()[:2], **kw)
    lats = lat[:1]
    with pytest.raises(NotImplementedError):
        ptp_utils.latent_step(ldm, ctrl, lats, [None, emb], ldm.scheduler.timesteps[0], 7.5, low_resource=False)


def test_load_ldm_prediction_type(tmp_path):
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.optimize_token import load_ldm
    import stablekeypoints_amd.ldm.pipeline as P
    unet, vae = StableDiffusionPipeline.build("tiny", seed=7)
    d = tmp_path / "tiny-ckpt"
    d.mkdir()
    torch.save(unet.state_dict(), str(d / "unet.pt"))
    torch.save(vae.state_dict(), str(d / "vae.pt"))
    orig = P.guess_arch
    P.guess_arch = lambda name: "tiny"
    try:
        ldm, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32)
        assert ldm.scheduler.prediction_type == "epsilon"                              # no scheduler config
        (d / "scheduler").mkdir()
        (d / "scheduler" / "scheduler_config.json").write_text(json.dumps({"prediction_type": "v_prediction"}))
        ldm, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32)
        assert ldm.scheduler.prediction_type == "v_prediction" and int(ldm.scheduler.timesteps[0]) == 980
        ldm, _, _ = load_ldm("cpu", str(d), feature_upsample_res=32, prediction_type="sample")
        assert ldm.scheduler.prediction_type == "sample"                               # the argument wins over the file
        with pytest.raises(ValueError):
            load_ldm("cpu", str(d), feature_upsample_res=32, prediction_type="velocity")
    finally:
        P.guess_arch = orig
    ldm, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=32)
    assert ldm.scheduler.prediction_type == "epsilon"                                  # synthetic architectures
    ldm, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, prediction_type="v_prediction")
    assert ldm.scheduler.prediction_type == "v_prediction"
