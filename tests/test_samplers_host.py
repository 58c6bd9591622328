"""CPU tests of the sampler plans (ldm/samplers.py: stochastic DDIM, DPM-Solver++(2M), SDE-DPM-Solver++(2M)) and of
`ptp_utils.text2image_ldm_stable(..., sampler=, eta=)` on the host route: the coefficients against an fp64 restatement written out
here, three identities that tie the samplers to the schedule, and the whole loop against the same loop on an fp64 copy of the
modules with the noise drawn the same way."""
import contextlib
import copy
import itertools
import math

import pytest
import torch

import _sampler_cases as C
from _sampler_cases import SAMPLERS, STEPS, T_TRAIN


def _close(got, want, rtol=1e-12):
    return got == want if want == 0 else abs(got - want) <= rtol * abs(want)


@pytest.mark.parametrize("n", [4, 20])
@pytest.mark.parametrize("alpha_to_one", [True, False])
def test_plan_coefficients_vs_fp64_restatement(n, alpha_to_one):
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    sched, acp, final = C.schedule(alpha_to_one)
    sched.set_timesteps(50)
    table = copy.deepcopy(sched)
    table.set_timesteps(n)
    for kind, eta in SAMPLERS + (("ddim", 0.0),):
        ts, rows = SamplerPlan(sched, kind, eta).plan(n)
        assert torch.equal(ts, table.timesteps) and ts.device.type == "cpu" and len(rows) == n      # every sampler visits the same t
        want = C.restated_rows(kind, eta, acp, final, n)
        for i, (g, w) in enumerate(zip(rows, want)):
            assert all(isinstance(v, float) for v in g) and len(g) == 7
            assert all(_close(a, b) for a, b in zip(g, w)), (kind, eta, i, tuple(g), w)
        if kind != "ddim":                                       # second-order steps in the middle, first-order ends
            assert rows[0].c1 == 0 and rows[-1].c1 == 0 and all(r.c1 != 0 for r in rows[1:-1])
            if alpha_to_one:
                assert rows[-1][2:] == (0.0, 1.0, 0.0, 0.0, 0.0)
    # the plan reads the scheduler and leaves it as it was
    assert sched.num_inference_steps == 50 and int(sched.timesteps[0]) == 980 and len(sched.timesteps) == 50


@pytest.mark.parametrize("n", [4, 20])
@pytest.mark.parametrize("alpha_to_one", [True, False])
def test_identities(n, alpha_to_one):
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    sched, acp, final = C.schedule(alpha_to_one)
    stride = T_TRAIN // n
    ts, ddim0 = SamplerPlan(sched, "ddim", 0.0).plan(n)
    _, dpm1 = SamplerPlan(sched, "dpm++2m", order=1).plan(n)
    _, sde = SamplerPlan(sched, "dpm++2m-sde").plan(n)
    for i, t in enumerate(ts.tolist()):
        ap = acp[t - stride] if t - stride >= 0 else final
        alpha, sigma, alpha_p, sigma_p = math.sqrt(acp[t]), math.sqrt(1 - acp[t]), math.sqrt(ap), math.sqrt(1 - ap)
        # 1. first-order DPM-Solver++ is DDIM with eta 0: the same (cx x + c0 x0) map, also into final_alpha_cumprod == 1
        assert dpm1[i].c1 == 0 and dpm1[i].ce == 0 and dpm1[i].cn == 0 and ddim0[i].cx == 0
        assert _close(dpm1[i].cx, ddim0[i].ce / sigma) and _close(dpm1[i].c0, alpha_p - sigma_p * alpha / sigma), (i, t)
        # 2. DDIM at any eta: ce^2 + cn^2 == 1 - a'; no noise at eta 0
        assert ddim0[i].cn == 0
        for eta in (0.0, 0.3, 0.5, 1.0):
            row = SamplerPlan(sched, "ddim", eta).plan(n)[1][i]
            assert abs(row.ce ** 2 + row.cn ** 2 - (1 - ap)) <= 1e-12 * (1 - ap), (eta, i)
        # 3. SDE-DPM-Solver++: the noise level after the step is the schedule's
        assert abs((sde[i].cx * sigma) ** 2 + sde[i].cn ** 2 - sigma_p ** 2) <= 1e-12 * sigma_p ** 2, (i, t)
    if alpha_to_one:
        assert dpm1[-1].cx == 0 and dpm1[-1].c0 == 1.0


def test_plan_errors():
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    sched, _, _ = C.schedule(False)
    for bad in ("euler", "DDIM", "", None):
        with pytest.raises(ValueError):
            SamplerPlan(sched, bad)
    for eta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SamplerPlan(sched, "ddim", eta)
    with pytest.raises(ValueError):
        SamplerPlan(sched, "dpm++2m", 0.5)                       # eta belongs to "ddim"
    for n in (0, -3):
        with pytest.raises(ValueError):
            SamplerPlan(sched, "dpm++2m").plan(n)
    assert len(SamplerPlan(sched, "dpm++2m").plan(1)[1]) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# the loop on CPU tensors: the reduced-width tree, 64^2 images (8^2 latents), 4 steps
# ---------------------------------------------------------------------------------------------------------------------------
# Tolerance: max |image - image64| / max |image64| <= 4x the same figure of the loop written out on the plain fp32 modules (no
# hooks, the modules' own forward) -- the rule and the constant of the existing whole-loop DDIM tests (tests/test_generate_gpu.py,
# tests/test_generate_guided_gpu.py: "the error of the EAGER fp32 modules' own loop against fp64, times 4"), with the host as the
# device.  The existing host files hold single steps to constants (1e-6, 1e-5 of the maximum) and have no whole-loop comparison to
# take a constant from: four forwards of this untrained tree under guidance 7.5 put the plain fp32 loop itself between 7e-7 and
# 2e-5 from fp64, case by case.  Latents and guidance scales: tests/_sampler_cases.py, picked from the fp64 loop alone
# (GAIN <= MAX_GAIN, asserted by test_cases_are_well_conditioned below).
EAGER_MARGIN = 4.0


@pytest.fixture(scope="module")
def trees():
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True)
    plain = StableDiffusionPipeline.from_pretrained("tiny", with_decoder=True)
    assert torch.equal(plain.unet.conv_in.weight, ldm.unet.conv_in.weight)                # the same seeded tree, without the hooks
    pipe64 = copy.deepcopy(plain)
    pipe64.unet.double(); pipe64.vae.double()
    return dict(ldm=ldm, ctrl=next(iter(controllers.values())), pipe64=pipe64, pipe32=plain, emb=C.embeddings())


@contextlib.contextmanager
def _scheduler(ldm, prediction, clip=False, alpha_to_one=False):
    """The model with a scheduler of the given kind (50-step table set, as load_ldm leaves it) -> (acp, final) in fp64."""
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    kept = ldm.scheduler
    ldm.scheduler = DDIMScheduler(clip_sample=clip, set_alpha_to_one=alpha_to_one, prediction_type=prediction, **C.SD)
    ldm.scheduler.set_timesteps(50)
    acp = ldm.scheduler.alphas_cumprod.double().tolist()
    try:
        yield acp, (1.0 if alpha_to_one else acp[0])
    finally:
        ldm.scheduler = kept


# every sampler x {unguided, guided} x {epsilon, v}, and the clamp together with the step into final_alpha_cumprod == 1
LOOP_CASES = [(s, e, g, p, False, False) for (s, e), g, p in itertools.product(SAMPLERS, (False, True), ("epsilon", "v_prediction"))]
LOOP_CASES += [(s, e, False, "epsilon", True, True) for s, e in C.CLIP_CASES]


# every whole-loop case of this file and of tests/test_samplers_gpu.py: (sampler, eta, prediction, uncond, seed, guidance, clip and alpha_to_one)
GAIN_CASES = [(s, e, p, "u16" if g else None) + C.case_inputs(s, e, g, p) + (c,) for s, e, g, p, c, _ in LOOP_CASES]
GAIN_CASES += [(s, e, "epsilon", "u24", C.SINGLE_SEED, C.GUIDANCE, False) for s, e in C.T24_SAMPLERS]
GAIN_CASES += [(s, e, "epsilon", u, seed, C.GUIDANCE, False) for (s, e), u, seed in itertools.product(SAMPLERS, (None, "u16"), C.BATCH_SEEDS)]
GAIN_CASES = list(dict.fromkeys(GAIN_CASES))                     # (a batch seed may be a single-image seed as well)


@pytest.mark.parametrize("sampler,eta,prediction,uncond,seed,guidance,clip", GAIN_CASES)
def test_cases_are_well_conditioned(trees, sampler, eta, prediction, uncond, seed, guidance, clip):
    """The criterion the latents and guidance scales were picked by, held: on the fp64 loop alone, GAIN <= MAX_GAIN for every
    whole-loop case the two sampler test files use.  A change of the seeded tree that moves a case out of it fails here, not as
    an unexplained miss of a 4x bound."""
    emb = trees["emb"]
    gain = C.gain(trees["pipe64"], sampler, eta, prediction, guidance, seed, None if uncond is None else emb[uncond], emb["cond"],
                  clip, clip)
    print(f"GAIN {sampler} eta={eta} {prediction} uncond={uncond} seed {seed} guidance {guidance} clip={clip}: {gain:.1f}")
    assert gain <= C.MAX_GAIN


@pytest.mark.parametrize("sampler,eta,guided,prediction,clip,alpha_to_one", LOOP_CASES)
def test_loop_on_cpu_vs_fp64_loop(trees, sampler, eta, guided, prediction, clip, alpha_to_one):
    from stablekeypoints_amd import ptp_utils, routes
    ldm, ctrl, emb = trees["ldm"], trees["ctrl"], trees["emb"]
    seed, guidance = C.case_inputs(sampler, eta, guided, prediction)
    latent, noise = C.draw(seed, C.stochastic(sampler, eta))
    extra = dict(uncond_embedding=emb["u16"], guidance_scale=guidance) if guided else {}
    with _scheduler(ldm, prediction, clip, alpha_to_one) as (acp, final):
        before = routes.snapshot()
        img, lat0 = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, num_inference_steps=STEPS, height=64, width=64,
                                                    generator=torch.Generator().manual_seed(seed), output_type="float",
                                                    sampler=sampler, eta=eta, **extra)
        d = routes.delta(before)
        assert int(ldm.scheduler.timesteps[0]) == 980 and ldm.scheduler.num_inference_steps == 50
        with torch.no_grad():
            args = (acp, final, prediction, clip, sampler, eta, latent, emb["cond"], emb["u16"] if guided else None, noise, guidance)
            ref = C.loop(trees["pipe64"], torch.float64, "cpu", *args)
            e_eager = C.rel(C.loop(trees["pipe32"], torch.float32, "cpu", *args).double(), ref)
    assert torch.equal(lat0, latent) and img.shape == (1, 3, 64, 64) and img.dtype == torch.float32
    assert d.get(("sample.step", "host"), 0) == STEPS and ("sample.step", "sampler_step") not in d
    assert not ctrl.step_store["attn"]
    err = C.rel(img.double(), ref)
    print(f"host loop {sampler} eta={eta} guided={guided} {prediction} clip={clip} (seed {seed}, guidance {guidance}): plain fp32 loop vs fp64 {e_eager:.3e}, "
          f"text2image_ldm_stable vs fp64 {err:.3e} (bound {EAGER_MARGIN * e_eager:.3e})")
    assert err <= EAGER_MARGIN * e_eager


@pytest.mark.parametrize("sampler,eta,guided", [(s, e, g) for (s, e), g in itertools.product(SAMPLERS, (False, True))])
def test_batch_rows_see_the_single_image_draws(trees, sampler, eta, guided):
    """Image i of a 2-image batch against its own fp64 loop and against the single-image call with generator[i]: the same latent
    and the same noise bit for bit (the draws are per image), the images within the sum of their two bounds (a batched forward
    sums in another order than a single-row one) -- the comparison of tests/test_generate_guided_gpu.py's batch test."""
    from stablekeypoints_amd import ptp_utils
    ldm, ctrl, emb = trees["ldm"], trees["ctrl"], trees["emb"]
    extra = dict(uncond_embedding=emb["u16"], guidance_scale=C.GUIDANCE) if guided else {}
    kw = dict(num_inference_steps=STEPS, height=64, width=64, output_type="float", sampler=sampler, eta=eta, **extra)
    with _scheduler(ldm, "epsilon") as (acp, final):
        img, lat = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, 
                                                   generator=[torch.Generator().manual_seed(s) for s in C.BATCH_SEEDS], **kw)
        assert img.shape == (2, 3, 64, 64) and lat.shape == (2, 4, 8, 8)
        for i, seed in enumerate(C.BATCH_SEEDS):
            latent, noise = C.draw(seed, C.stochastic(sampler, eta))
            assert torch.equal(lat[i:i + 1], latent)
            with torch.no_grad():
                args = (acp, final, "epsilon", False, sampler, eta, latent, emb["cond"], emb["u16"] if guided else None, noise, C.GUIDANCE)
                ref = C.loop(trees["pipe64"], torch.float64, "cpu", *args)
                e_eager = C.rel(C.loop(trees["pipe32"], torch.float32, "cpu", *args).double(), ref)
            one, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, generator=torch.Generator().manual_seed(seed), **kw)
            e_row, e_one = C.rel(img[i:i + 1].double(), ref), C.rel(one.double(), ref)
            print(f"host batch {sampler} eta={eta} guided={guided} row {i} (seed {seed}): plain fp32 single-image loop vs fp64 "
                  f"{e_eager:.3e}, batched row vs fp64 {e_row:.3e}, single call vs fp64 {e_one:.3e} (bound {EAGER_MARGIN * e_eager:.3e})")
            assert e_row <= EAGER_MARGIN * e_eager and e_one <= EAGER_MARGIN * e_eager
            assert (img[i:i + 1] - one).abs().max().item() <= 2 * EAGER_MARGIN * e_eager * ref.abs().max().item()
        if C.stochastic(sampler, eta):                            # a given latent with the generators: the same noise, the same image
            again, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, latent=lat,
                                                       generator=[_after_latent(s) for s in C.BATCH_SEEDS], **kw)
            assert torch.equal(again, img)


def _after_latent(seed):
    g = torch.Generator().manual_seed(seed)
    torch.randn((1, 4, 8, 8), generator=g)
    return g


def test_default_call_unchanged_and_errors(trees):
    from stablekeypoints_amd import ptp_utils, routes
    ldm, ctrl, emb = trees["ldm"], trees["ctrl"], trees["emb"]
    lat = torch.cat([C.draw(s, False)[0] for s in C.BATCH_SEEDS])
    kw = dict(num_inference_steps=STEPS, height=64, width=64, latent=lat, output_type="float")
    for extra in ({}, dict(uncond_embedding=emb["u16"], guidance_scale=C.GUIDANCE)):
        before = routes.snapshot()
        a, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, **kw, **extra)
        b, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, sampler=None, **kw, **extra)
        c, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, sampler="ddim", eta=0.0, **kw, **extra)
        assert torch.equal(a, b) and torch.equal(a, c)            # None, and "ddim" at eta 0: the step the call always had
        assert not [k for k in routes.delta(before) if k[0] == "sample.step"]
        d, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, sampler="dpm++2m", **kw, **extra)
        assert not torch.equal(a, d)
    assert routes.ROUTES["sample.step"] == {"sampler_step": "hip", "host": "host"}
    for bad in (dict(sampler="euler"), dict(sampler="ddim", eta=1.5), dict(sampler="ddim", eta=-0.5), dict(sampler="dpm++2m", eta=2.0),
                dict(eta=0.5), dict(sampler=None, eta=1.0), dict(sampler="dpm++2m-sde", eta=0.5)):   # eta without "ddim" is not ignored
        with pytest.raises(ValueError):
            ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, **kw, **bad)
    for stochastic in (dict(sampler="ddim", eta=0.5), dict(sampler="dpm++2m-sde")):
        with pytest.raises(ValueError, match="generator"):       # a given latent and nothing to draw the noise from
            ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, **kw, **stochastic)
        with pytest.raises(ValueError, match="generator"):       # one generator for two rows
            ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, generator=torch.Generator().manual_seed(1), **kw, **stochastic)
    with pytest.raises(TypeError):                               # keyword-only
        ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, STEPS, 7.5, None, lat, "dpm++2m")
    assert int(ldm.scheduler.timesteps[0]) == 980 and not ctrl.step_store["attn"]
