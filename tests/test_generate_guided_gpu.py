"""Guided / batched / v-prediction image sampling on the MI355X: the step kernel (csrc/skp_sampler_step.hip) against the fp64 formula
with a derived per-element bound, the image-to-bytes kernel bit for bit, and `ptp_utils.text2image_ldm_stable` with guidance, batches
and the three prediction types against the same loop on an fp64 host copy of the modules.

Module tolerances follow tests/test_generate_gpu.py: the error of the EAGER fp32 modules' own loop on the GPU against fp64, times 4.
The measured figures are recorded in profiles/generate_guided.md."""
import copy
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
STEPS = 4
KINDS = ("epsilon", "v_prediction", "sample")


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the step kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _step_coefficients():
    """(label, sa, sb, pa, pb) in fp64 at the first and the last step of the 4-step and the 50-step tables: sa is smallest at
    t = 980, sb at t = 0, where prev_t < 0."""
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    out = []
    for n_steps in (4, 50):
        s = DDIMScheduler(**SD)
        s.set_timesteps(n_steps)
        for t in (int(s.timesteps[0]), int(s.timesteps[-1])):
            out.append((f"{n_steps} steps t={t}",) + tuple(s._coefficients(t)))
    assert out[2][0] == "50 steps t=980" and out[1][0] == "4 steps t=0"
    return out


def _ref64(x, mc, mu, g, kind, clip, sa, sb, pa, pb):
    """-> (y, S) in fp64: the formula of include/skp.h and the magnitude sum its roundings are relative to."""
    x, mc = x.double(), mc.double()
    if mu is None:
        m, M = mc, mc.abs()
    else:
        mu = mu.double()
        m, M = mu + g * (mc - mu), mu.abs() + abs(g) * (mc.abs() + mu.abs())
    ax = x.abs()
    if kind == 0:
        x0, eps, X0, E = (x - sb * m) / sa, m, (ax + sb * M) / sa, M
    elif kind == 1:
        x0, eps, X0, E = sa * x - sb * m, sa * m + sb * x, sa * ax + sb * M, sa * M + sb * ax
    else:
        x0, eps, X0, E = m, (x - sa * m) / sb, M, (ax + sa * M) / sb
    if clip:
        x0 = x0.clamp(-1, 1)
    return pa * x0 + pb * eps, pa * X0 + pb * E


UNITS = 16.0          # roundings on the longest chain: 3 guidance mix + 4 coefficients + <= 5 for x0 and eps + 2 final mix = 14


@pytest.mark.parametrize("n", [1, 5, 768, 1023, 16387])
def test_ddim_step_vs_fp64(ops, n):
    """Every prediction type x clip x guidance x copies x step, on inputs of mixed scale; per element |y - y64| <= 16 * 2^-24 * S.
    Worst case measured on the MI355X: see profiles/generate_guided.md."""
    gen = torch.Generator().manual_seed(100 + n)
    scale = torch.tensor([0.1, 1.0, 4.0])[torch.arange(n) % 3]
    worst = (0.0, None)
    for noise in (0.01, 1.0):
        x = torch.randn(n, generator=gen) * scale
        mc = torch.randn(n, generator=gen)
        mu = mc + noise * torch.randn(n, generator=gen)
        xg, mcg, mug = x.cuda(), mc.cuda(), mu.cuda()
        for (label, sa, sb, pa, pb), kind, clip, g, copies in itertools.product(_step_coefficients(), (0, 1, 2), (False, True),
                                                                                (None, 7.5, 0.0, 1.0, -2.0), (1, 2)):
            y = ops.ddim_step(xg, mcg, None if g is None else mug, sa=sa, sb=sb, pa=pa, pb=pb, guidance=1.0 if g is None else g,
                              prediction=kind, clip=clip, copies=copies)
            assert y.shape == (copies * n,)
            if copies == 2:
                assert torch.equal(y[:n], y[n:])
            ref, S = _ref64(x, mc, None if g is None else mu, g, kind, clip, sa, sb, pa, pb)
            units = ((y[:n].cpu().double() - ref).abs() / (2.0 ** -24 * S)).max().item()
            if units > worst[0]:
                worst = (units, (label, kind, clip, g, copies, noise))
            assert units <= UNITS, (units, label, kind, clip, g, copies, noise)
    print(f"ddim_step n={n}: worst error {worst[0]:.2f} units of 2^-24 S at {worst[1]} (bound {UNITS:.0f})")


def test_ddim_step_aliasing_unaligned_and_determinism(ops):
    n = 1023
    gen = torch.Generator().manual_seed(9)
    x, mc, mu = (torch.randn(n, generator=gen).cuda() for _ in range(3))
    _, sa, sb, pa, pb = _step_coefficients()[2]
    for kind, clip in itertools.product((0, 1, 2), (False, True)):
        kw = dict(sa=sa, sb=sb, pa=pa, pb=pb, guidance=7.5, prediction=kind, clip=clip)
        y = ops.ddim_step(x, mc, mu, **kw)
        assert torch.equal(y, ops.ddim_step(x, mc, mu, **kw))                       # two runs: the same bits
        xa = x.clone()
        assert ops.ddim_step(xa, mc, mu, out=xa, **kw) is xa and torch.equal(xa, y)  # y is x
        buf = torch.empty(2 * n, device="cuda")
        buf[:n] = x
        ops.ddim_step(buf[:n], mc, mu, copies=2, out=buf, **kw)                      # x is the first copy
        assert torch.equal(buf[:n], y) and torch.equal(buf[n:], y)
        # views one float past a 16-byte boundary: the scalar form, held to the same bound
        ref, S = _ref64(x.cpu(), mc.cpu(), mu.cpu(), 7.5, kind, clip, sa, sb, pa, pb)
        for which in range(4):
            t = [x, mc, mu, None]
            if which < 3:
                base = torch.empty(n + 1, device="cuda")
                base[1:] = t[which]
                t[which] = base[1:]
                assert t[which].data_ptr() % 16 == 4
                yo = ops.ddim_step(t[0], t[1], t[2], **kw)
            else:
                base = torch.full((2 * n + 1,), float("nan"), device="cuda")
                yo = ops.ddim_step(x, mc, mu, copies=2, out=base[1:], **kw)
                assert torch.equal(yo[:n], yo[n:]) and bool(torch.isnan(base[0]))
                yo = yo[:n]
            assert ((yo.cpu().double() - ref).abs() / (2.0 ** -24 * S)).max().item() <= UNITS
    with pytest.raises(RuntimeError):
        ops.ddim_step(x, mc[:-1], mu, sa=sa, sb=sb, pa=pa, pb=pb)
    with pytest.raises(ValueError):
        ops.ddim_step(x, mc, mu, sa=sa, sb=sb, pa=pa, pb=pb, prediction="velocity")


def test_ddim_step_and_image_u8_c_abi(ops):
    lib = ops.N.lib()
    buf = torch.zeros(64, device="cuda")
    p, BAD = buf.data_ptr(), -1
    co = (1.0, 0, 0.9, 0.4, 0.95, 0.3, 0)                      # guidance, prediction, sa, sb, pa, pb, clip
    assert lib.skp_ddim_step_f32(None, p, None, p, 4, 1, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, None, None, p, 4, 1, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, None, None, 4, 1, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, 0, 1, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, -4, 1, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, 4, 0, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, 4, 3, *co, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, 4, 1, 1.0, 3, 0.9, 0.4, 0.95, 0.3, 0, None) == BAD
    assert lib.skp_ddim_step_f32(p, p, p, p, 4, 1, 1.0, -1, 0.9, 0.4, 0.95, 0.3, 0, None) == BAD
    assert lib.skp_image_u8_nhwc_f32(None, p, 1, 2, 2, None) == BAD
    assert lib.skp_image_u8_nhwc_f32(p, None, 1, 2, 2, None) == BAD
    assert lib.skp_image_u8_nhwc_f32(p, p, 0, 2, 2, None) == BAD
    assert lib.skp_image_u8_nhwc_f32(p, p, 1, 0, 2, None) == BAD
    assert lib.skp_image_u8_nhwc_f32(p, p, 1, 2, -2, None) == BAD
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(64))              # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------
# 2. image to bytes
# ---------------------------------------------------------------------------------------------------------------------------
def _host_u8(image):
    return (image.cpu().permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)


# odd plane (one pixel per lane); planes that are multiples of four (four pixels per lane), one and several images
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 64, 64), (3, 3, 16, 24)])
def test_image_u8_is_exact(ops, shape):
    k = torch.arange(256, dtype=torch.float64) / 255
    k32 = k.float()
    special = torch.cat([torch.tensor([0.0, 1.0, 1.0 - 2.0 ** -24]), k32, torch.nextafter(k32, torch.tensor(2.0)),
                         torch.nextafter(k32, torch.tensor(-1.0))]).clamp(0, 1)
    numel = int(np.prod(shape))
    gen = torch.Generator().manual_seed(numel)
    if numel >= 2 * special.numel():                             # every special value, the rest random, shuffled
        vals = torch.cat([special, torch.rand(numel - special.numel(), generator=gen)])
    else:                                                        # the small shape: a random half of special values, half random
        pick = special[torch.randperm(special.numel(), generator=gen)[:numel // 2 - 3]]
        vals = torch.cat([special[:3], pick, torch.rand(numel - numel // 2, generator=gen)])
    vals = vals[torch.randperm(numel, generator=gen)].reshape(shape)
    assert float(vals.min()) == 0.0 and float(vals.max()) == 1.0
    y = ops.image_u8_nhwc(vals.cuda())
    assert y.shape == (shape[0], shape[2], shape[3], 3) and y.dtype == torch.uint8 and y.is_cuda
    assert np.array_equal(y.cpu().numpy(), _host_u8(vals))
    with pytest.raises(RuntimeError):
        ops.image_u8_nhwc(torch.zeros(1, 4, 8, 8, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------
# 3 - 6. module level: the reduced-width tree, 64^2 images (8^2 latents), 4 steps
# ---------------------------------------------------------------------------------------------------------------------------
def _loop(pipe, dtype, device, acp, latent, cond, uncond, g, kind):
    """The sampling loop on a pipeline's own modules: the UNet forward(s), the guidance mix, the closed-form step of `kind`,
    the decode and the [0, 1] map.  Contexts of equal length share one forward of 2n rows; others take two."""
    lat = latent.to(device=device, dtype=dtype)
    n = lat.shape[0]
    c = cond.to(device=device, dtype=dtype).expand(n, -1, -1)
    u = None if uncond is None else uncond.to(device=device, dtype=dtype).expand(n, -1, -1)
    for t in (torch.arange(0, STEPS) * (1000 // STEPS)).flip(0):
        if u is None:
            m = pipe.unet(lat, t, c)["sample"]
        else:
            if u.shape[1] == c.shape[1]:
                both = pipe.unet(torch.cat([lat, lat]), t, torch.cat([u, c]))["sample"]
                mu, mc = both[:n], both[n:]
            else:
                mu, mc = pipe.unet(lat, t, u)["sample"], pipe.unet(lat, t, c)["sample"]
            m = mu + g * (mc - mu)
        t_, p_ = int(t), int(t) - 1000 // STEPS
        a_t, a_p = float(acp[t_]), float(acp[p_]) if p_ >= 0 else float(acp[0])
        sa, sb, pa, pb = a_t ** 0.5, (1 - a_t) ** 0.5, a_p ** 0.5, (1 - a_p) ** 0.5
        if kind == "epsilon":
            x0, eps = (lat - sb * m) / sa, m
        elif kind == "v_prediction":
            x0, eps = sa * lat - sb * m, sa * m + sb * lat
        else:
            x0, eps = m, (lat - sa * m) / sb
        lat = pa * x0 + pb * eps
    return (pipe.vae.decode(lat / 0.18215)["sample"] / 2 + 0.5).clamp(0, 1)


GUIDANCE = 7.5
# Which latents.  The seeded reduced-width UNet is no trained denoiser: on some latents four steps (under guidance 7.5 above all)
# amplify a change of the input by hundreds, and then any two fp32 evaluations of the loop -- the eager modules' included -- lie
# that factor apart by chance and "4x the eager error" measures luck.  The criterion is taken from the fp64 host loop alone: GAIN =
# (max change of the fp64 image / its max) / 2^-24 when every element of the latent is changed by a random relative 2^-24, the
# largest of four such draws (one draw is not enough: seed 41 shows 2.7 on one and 39.9 on another).  Over the seeds 40 .. 60 it
# ranges from 1.1 to 5112.  Used: torch.randn((1, 4, 8, 8), manual_seed(s)) for
#   s = 43, 48, 57 -- the batch: the first three seeds from 40 on with GAIN <= 8 for the plain and the guided loop
#                     (1.2 / 4.0, 1.2 / 2.9, 1.6 / 4.0; 40, 41, 42, 44 .. 47 have 13 .. 5112 on one of the two);
#   s = 58 -- the single-image cases: guided 5.3, guided with 24 tokens 2.4, v 3.1, sample 11.4 -- the one seed measured on which
#             all four stay under 16 (the sample-prediction loop has 30 .. 2610 on 43, 48, 57, 60).
SINGLE_SEED, BATCH_SEEDS = 58, (43, 48, 57)
# name -> (prediction type, unconditional embedding: None / "u16" / "u24")
CASES = {
    "plain": ("epsilon", None),
    "guided": ("epsilon", "u16"),
    "guided_t24": ("epsilon", "u24"),
    "v": ("v_prediction", None),
    "sample": ("sample", None),
}


def _latent(seed):
    return torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def trees():
    """One fused pipeline per prediction type on the GPU, the same modules eager on the GPU and in fp64 on the host, and for every
    case and latent the single-image reference loops (fp64, and eager fp32 for the yardstick).  All hold the same seeded weights; the
    references are computed once here and only read by the tests.  The eager loops run under the library's fixed-summation-order
    convolution solvers, as the sampling call itself does: the yardstick is the same number in every run."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    from stablekeypoints_amd.optimize_token import load_ldm
    fused = {}
    for kind in KINDS:
        ldm, controllers, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True, prediction_type=kind)
        assert ldm.scheduler.prediction_type == kind
        fused[kind] = (ldm, next(iter(controllers.values())))
    plain = StableDiffusionPipeline.from_pretrained("tiny", scheduler=DDIMScheduler(**SD), with_decoder=True)
    for k, v in fused["epsilon"][0].unet.state_dict().items():
        assert torch.equal(v.cpu(), plain.unet.state_dict()[k]), k
    acp = plain.scheduler.alphas_cumprod.double()
    cpu64 = copy.deepcopy(plain)
    cpu64.unet.double(); cpu64.vae.double()
    eager = plain.to("cuda")
    g = torch.Generator().manual_seed(23)
    emb = dict(cond=torch.randn(1, 16, 768, generator=g), u16=torch.randn(1, 16, 768, generator=g),
               u24=torch.randn(1, 24, 768, generator=g))
    ref = {}
    with torch.no_grad(), ptp_utils._reproducible_library_convolutions():
        for name, (kind, unc) in CASES.items():
            u = None if unc is None else emb[unc]
            for seed in (BATCH_SEEDS if name == "plain" else (SINGLE_SEED,) + BATCH_SEEDS if name == "guided" else (SINGLE_SEED,)):
                lat = _latent(seed)
                r64 = _loop(cpu64, torch.float64, "cpu", acp, lat, emb["cond"], u, GUIDANCE, kind)
                re = _loop(eager, torch.float32, "cuda", acp, lat, emb["cond"], u, GUIDANCE, kind).cpu().double()
                ref[(name, seed)] = (r64, _rel(re, r64))
    return dict(fused=fused, emb=emb, ref=ref, ptp=ptp_utils)


def _rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def _sample(trees, name, latent, **kw):
    kind, unc = CASES[name]
    ldm, ctrl = trees["fused"][kind]
    extra = {} if unc is None else dict(uncond_embedding=trees["emb"][unc], guidance_scale=GUIDANCE)
    out = trees["ptp"].text2image_ldm_stable(ldm, trees["emb"]["cond"], ctrl, num_inference_steps=STEPS, height=64, width=64,
                                             latent=latent, **extra, **kw)
    assert not ctrl.step_store["attn"]                          # the hooked store is left empty
    assert int(ldm.scheduler.timesteps[0]) == 980               # the optimisation path's 50-step table is back
    return out


@pytest.mark.parametrize("name", ["guided", "guided_t24", "v", "sample"])
def test_guided_and_prediction_types_vs_fp64_loop(trees, tune, name):
    """One image, 4 steps at 64^2 from a given latent: classifier-free guidance with contexts of equal (one 2-row forward) and of
    different length (two forwards), and v / sample prediction, each against the same loop on the fp64 host copy; tolerance 4x
    the eager fp32 loop's own error.  (v / sample prediction UNDER guidance is held to the fp64 formula per element in
    test_ddim_step_vs_fp64; as a whole loop on this tree its GAIN (below) is above 100 on every latent tried, nothing to hold a bound
    against.)  Figures: profiles/generate_guided.md."""
    tune("conv_up2", 1)                                         # as tests/test_generate_gpu.py: the 32-channel up-samplers on the own kernel
    lat = _latent(SINGLE_SEED)
    img, lat0 = _sample(trees, name, lat, output_type="float")
    r64, e_eager = trees["ref"][(name, SINGLE_SEED)]
    assert img.shape == (1, 3, 64, 64) and img.is_cuda and torch.equal(lat0, lat)
    e_fused = _rel(img.cpu().double(), r64)
    print(f"sampling tiny 4 steps 64^2 [{name}]: eager fp32 loop vs fp64 {e_eager:.3e}, fused vs fp64 {e_fused:.3e} "
          f"(bound {4 * e_eager:.3e})")
    assert e_fused <= 4 * e_eager


@pytest.mark.parametrize("name", ["plain", "guided"])
def test_batch_rows_vs_their_own_fp64_loops(trees, tune, name):
    """Three images in one call: row i against its own fp64 single-image loop, bound 4x the error of the eager fp32 modules'
    single-image loop on that latent -- the rule of test_sampling_vs_fp64_loop; the single-image call from latent[i] is held to
    the same bound, and the two agree within the sum of their bounds.  Figures on the MI355X: profiles/generate_guided.md."""
    tune("conv_up2", 1)
    lat = torch.cat([_latent(s) for s in BATCH_SEEDS])
    img, lat0 = _sample(trees, name, lat, output_type="float")
    assert img.shape == (3, 3, 64, 64) and torch.equal(lat0, lat)
    for i, seed in enumerate(BATCH_SEEDS):
        r64, e_eager = trees["ref"][(name, seed)]
        e_row = _rel(img[i:i + 1].cpu().double(), r64)
        one, _ = _sample(trees, name, lat[i:i + 1], output_type="float")
        e_one = _rel(one.cpu().double(), r64)
        apart = _rel(img[i:i + 1].cpu().double(), one.cpu().double())
        print(f"batch of 3 [{name}] row {i} (seed {seed}): eager single-image loop vs fp64 {e_eager:.3e}, "
              f"fused batched row vs fp64 {e_row:.3e}, fused single call vs fp64 {e_one:.3e} (bound {4 * e_eager:.3e}); fused "
              f"batched row vs fused single call {apart:.3e}")
        assert e_row <= 4 * e_eager and e_one <= 4 * e_eager
        assert (img[i:i + 1] - one).abs().max().item() <= 8 * e_eager * r64.abs().max().item()
    ldm, ctrl = trees["fused"]["epsilon"]
    kw = dict(num_inference_steps=STEPS, height=64, width=64)
    extra = {} if name == "plain" else dict(uncond_embedding=trees["emb"]["u16"], guidance_scale=GUIDANCE)
    gens = [torch.Generator().manual_seed(s) for s in (4, 5, 6)]
    u8, lat3 = trees["ptp"].text2image_ldm_stable(ldm, trees["emb"]["cond"], ctrl, generator=gens, **extra, **kw)
    assert u8.shape == (3, 64, 64, 3) and str(u8.dtype) == "uint8" and lat3.shape == (3, 4, 8, 8)
    assert torch.equal(lat3[1:2], torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(5)))


def test_defaults_unchanged_and_latent2image_on_the_device(trees):
    """A call without the new arguments: equal bits from call to call, shapes of one image, the step on `ops.axpby`; the uint8
    image made on the device equals the host expression applied to the float image."""
    from stablekeypoints_amd import routes
    ldm, ctrl = trees["fused"]["epsilon"]
    ptp, emb, lat = trees["ptp"], trees["emb"]["cond"], _latent(SINGLE_SEED)
    kw = dict(num_inference_steps=STEPS, height=64, width=64)
    a, _ = ptp.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, output_type="float", **kw)
    b, _ = ptp.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, output_type="float", **kw)
    assert a.shape == (1, 3, 64, 64) and torch.equal(a, b)
    assert not ctrl.step_store["attn"] and int(ldm.scheduler.timesteps[0]) == 980
    before = routes.snapshot()
    u8, _ = ptp.text2image_ldm_stable(ldm, emb, ctrl, latent=lat, **kw)
    assert routes.delta(before).get(("image.u8", "nhwc_u8"), 0) == 1 and ("image.u8", "host") not in routes.delta(before)
    assert u8.shape == (1, 64, 64, 3) and np.array_equal(u8, _host_u8(a))
    z = torch.cat([_latent(s) for s in BATCH_SEEDS]).cuda()
    with torch.no_grad():
        want = _host_u8(ptp._latent2float(ldm.vae, z))
    assert np.array_equal(ptp.latent2image(ldm.vae, z), want)
    # the unguided epsilon step without clipping is still the two-coefficient pass, bit for bit
    from stablekeypoints_amd import ops
    x, m = torch.randn(2, 4, 8, 8, device="cuda"), torch.randn(2, 4, 8, 8, device="cuda")
    sa, sb, pa, pb = ldm.scheduler._coefficients(980)
    assert torch.equal(ldm.scheduler.step(m, 980, x)["prev_sample"], ops.axpby(x, m, pa / sa, pb - pa * sb / sa))
