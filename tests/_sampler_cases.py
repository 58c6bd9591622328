"""What tests/test_samplers_host.py and tests/test_samplers_gpu.py share: the samplers' coefficient rows restated in fp64 from their
definitions, the sampling loop written out on a pipeline's own modules (fp64 on the host as the reference; the eager fp32 modules on
the GPU as the yardstick), the draws of one image from its generator, and the inputs of the whole-loop cases.  Nothing here calls
stablekeypoints_amd.ldm.samplers."""
from __future__ import annotations

import math

import torch

SD = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
T_TRAIN = 1000
STEPS = 4                      # the first step, two second-order steps and the lower-order last step
SAMPLERS = (("ddim", 0.5), ("ddim", 1.0), ("dpm++2m", 0.0), ("dpm++2m-sde", 0.0))          # name, eta

# Which latents and which guidance.  The seeded reduced-width UNet is no trained denoiser: some loops amplify a rounding by hundreds
# or more, and then two fp32 evaluations of one loop lie that factor apart by chance (tests/test_generate_guided_gpu.py, whose
# criterion this extends).  GAIN = (max change of the fp64 image / its max) / 2^-24 when every element of the latent, and of the
# state after every step, is changed by a random relative 2^-24; the largest of GAIN_DRAWS draws, taken from the fp64 loop below
# alone with the noise of the case held fixed.  A case is used where GAIN <= MAX_GAIN, which tests/test_samplers_host.py asserts for
# every case (test_cases_are_well_conditioned).  `python tests/_sampler_cases.py` prints the figures; they are recorded in
# profiles/generate_samplers.md.  What the criterion turned down, of what was tried:
# seed 58 of the sibling tests (unguided "dpm++2m": 8.6 on four draws, 24.6 on 32, where the seeds used here have 3 to 4); guided
# "ddim" eta 0.5 on seed 43 (408); v prediction under guidance 7.5 on every seed tried (20 .. 119 949, as profiles/generate_guided.md
# says of the DDIM loop), hence its guidance of 2, and no single seed on which all four samplers pass under it.
GUIDANCE = 7.5
GAIN_DRAWS, MAX_GAIN = 8, 8.0
SINGLE_SEED = 50                                         # epsilon prediction: unguided, guided by 16 and by 24 tokens
# The batch runs every sampler unguided and guided on each of its seeds, so they are picked by a second measure of the reference's
# own as well: the error of the plain fp32 modules' loop on the host against fp64, the worst of those eight loops (it sees what
# roundings INSIDE a forward do under guidance 7.5, which GAIN's shaken state does not: seed 48 has GAIN <= 3.9 and 1.5e-05
# there).  Of the seeds 40 .. 79 the two smallest with GAIN <= MAX_GAIN: 62 (3.2e-06) and 50 (1.1e-05); 58 (5.2e-06) and 54 (1.1e-05)
# rank between them and have GAIN 8.6 and 12.7; the other 35 seeds have 1.2e-05 .. 5.7e-03.
BATCH_SEEDS = (50, 62)
V_GUIDED_GUIDANCE = 2.0
# v prediction: sampler -> (seed unguided, seed guided by 16 tokens at V_GUIDED_GUIDANCE)
V_SEEDS = {("ddim", 0.5): (57, 57), ("ddim", 1.0): (57, 57), ("dpm++2m", 0.0): (58, 43), ("dpm++2m-sde", 0.0): (57, 48)}
T24_SAMPLERS = (("dpm++2m", 0.0),)                       # guided by 24 tokens (two forwards per step): one sampler is enough


def case_inputs(sampler, eta, guided, prediction):
    """-> (latent seed, guidance scale) of a single-image whole-loop case."""
    if prediction == "epsilon":
        return SINGLE_SEED, GUIDANCE
    return (V_SEEDS[(sampler, eta)][1], V_GUIDED_GUIDANCE) if guided else (V_SEEDS[(sampler, eta)][0], GUIDANCE)


def stochastic(sampler, eta):
    return sampler == "dpm++2m-sde" or eta > 0


def schedule(alpha_to_one, **kw):
    """-> (scheduler, alphas_cumprod in fp64 as a list, final_alpha_cumprod) of the SD schedule."""
    from stablekeypoints_amd.ldm.scheduler import DDIMScheduler
    s = DDIMScheduler(set_alpha_to_one=alpha_to_one, **{"clip_sample": False, **kw}, **SD)
    acp = s.alphas_cumprod.double().tolist()
    return s, acp, (1.0 if alpha_to_one else acp[0])


def restated_rows(kind, eta, acp, final, n, first_order=False):
    """[(sa, sb, cx, c0, ce, c1, cn)] per step in fp64, from the formulas of the sampler's definition."""
    stride = T_TRAIN // n
    rows, h_prev = [], None
    for i, t in enumerate(reversed([k * stride for k in range(n)])):
        a, ap = acp[t], (acp[t - stride] if t - stride >= 0 else final)
        alpha, sigma, alpha_p, sigma_p = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(1 - ap)
        if kind == "ddim":
            s = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap)
            rows.append((alpha, sigma, 0.0, alpha_p, math.sqrt(1 - ap - s ** 2), 0.0, s))
            continue
        if sigma_p == 0:                                         # h is infinite: x' = alpha' x0
            rows.append((alpha, sigma, 0.0, alpha_p, 0.0, 0.0, 0.0))
            h_prev = None
            continue
        h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
        if kind == "dpm++2m":
            cx, cd, cn = sigma_p / sigma, -alpha_p * math.expm1(-h), 0.0
        else:
            cx, cd, cn = sigma_p / sigma * math.exp(-h), alpha_p * (1 - math.exp(-2 * h)), sigma_p * math.sqrt(1 - math.exp(-2 * h))
        if first_order or i == 0 or i == n - 1:
            rows.append((alpha, sigma, cx, cd, 0.0, 0.0, cn))
        else:
            r = h_prev / h
            rows.append((alpha, sigma, cx, cd * (1 + 1 / (2 * r)), 0.0, -cd / (2 * r), cn))
        h_prev = h
    return rows


def draw(seed, with_noise):
    """(latent, noise) of one image from its generator: the latent first, then one gaussian per step ([STEPS, 1, 4, 8, 8])."""
    g = torch.Generator().manual_seed(seed)
    latent = torch.randn((1, 4, 8, 8), generator=g)
    noise = torch.stack([torch.randn((1, 4, 8, 8), generator=g) for _ in range(STEPS)]) if with_noise else None
    return latent, noise


def loop(pipe, dtype, device, acp, final, prediction, clip, sampler, eta, latent, cond, uncond, noise, guidance=GUIDANCE, jitter=None):
    """The sampling loop written out on a pipeline's own modules: the UNet forward(s) (contexts of equal length share one forward of
    2n rows, others take two), the guidance mix, (x0, eps) by `prediction`, the optional clamp, the sampler's update from its
    definition with fp64 host numbers, the decode and the [0, 1] map.  `noise` [STEPS, n, C, h, w] or None.  `jitter` (a generator;
    the GAIN measurement): every element of the latent, and of the state after each step but the last, is changed by a random
    relative 2^-24 -- what rounding the state to fp32 once per step would do."""
    def shake(v):
        return v if jitter is None else v * (1 + 2.0 ** -24 * (2 * torch.rand(v.shape, generator=jitter, dtype=torch.float64).to(v) - 1))
    lat = shake(latent.to(device=device, dtype=dtype))
    n = lat.shape[0]
    c = cond.to(device=device, dtype=dtype).expand(n, -1, -1)
    u = None if uncond is None else uncond.to(device=device, dtype=dtype).expand(n, -1, -1)
    noise = None if noise is None else noise.to(device=device, dtype=dtype)
    stride = T_TRAIN // STEPS
    x0_prev = h_prev = None
    for i, t in enumerate(reversed([k * stride for k in range(STEPS)])):
        tt = torch.tensor(t)
        if u is None:
            m = pipe.unet(lat, tt, c)["sample"]
        else:
            if u.shape[1] == c.shape[1]:
                both = pipe.unet(torch.cat([lat, lat]), tt, torch.cat([u, c]))["sample"]
                mu, mc = both[:n], both[n:]
            else:
                mu, mc = pipe.unet(lat, tt, u)["sample"], pipe.unet(lat, tt, c)["sample"]
            m = mu + guidance * (mc - mu)
        a, ap = acp[t], (acp[t - stride] if t - stride >= 0 else final)
        alpha, sigma, alpha_p, sigma_p = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(1 - ap)
        if prediction == "epsilon":
            x0, eps = (lat - sigma * m) / alpha, m
        elif prediction == "v_prediction":
            x0, eps = alpha * lat - sigma * m, alpha * m + sigma * lat
        else:
            x0, eps = m, (lat - alpha * m) / sigma
        if clip:
            x0 = x0.clamp(-1, 1)
        if sampler == "ddim":
            s = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(1 - a / ap)
            lat = alpha_p * x0 + math.sqrt(1 - ap - s ** 2) * eps
            if s:
                lat = lat + s * noise[i]
        elif sigma_p == 0:
            lat = alpha_p * x0
        else:
            h = math.log(alpha_p / sigma_p) - math.log(alpha / sigma)
            if i == 0 or i == STEPS - 1:
                d = x0
            else:
                r = h_prev / h
                d = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * x0_prev
            if sampler == "dpm++2m":
                lat = (sigma_p / sigma) * lat - alpha_p * math.expm1(-h) * d
            else:
                lat = (sigma_p / sigma) * math.exp(-h) * lat + alpha_p * (1 - math.exp(-2 * h)) * d \
                    + sigma_p * math.sqrt(1 - math.exp(-2 * h)) * noise[i]
            h_prev = h
        x0_prev = x0
        if i < STEPS - 1:
            lat = shake(lat)
    return (pipe.vae.decode(lat / 0.18215)["sample"] / 2 + 0.5).clamp(0, 1)


def rel(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def embeddings():
    """The contexts of tests/test_generate_guided_gpu.py: cond and u16 of 16 tokens, u24 of 24."""
    g = torch.Generator().manual_seed(23)
    return dict(cond=torch.randn(1, 16, 768, generator=g), u16=torch.randn(1, 16, 768, generator=g),
                u24=torch.randn(1, 24, 768, generator=g))


def gain(pipe64, sampler, eta, prediction, guidance, seed, uncond, cond, clip=False, alpha_to_one=False):
    """GAIN of one case (see the top of this file), from the fp64 modules alone."""
    _, acp, final = schedule(alpha_to_one)
    latent, noise = draw(seed, stochastic(sampler, eta))
    with torch.no_grad():
        args = (pipe64, torch.float64, "cpu", acp, final, prediction, clip, sampler, eta, latent, cond, uncond, noise, guidance)
        ref = loop(*args)
        return max(rel(loop(*args, jitter=torch.Generator().manual_seed(1000 + k)), ref) / 2.0 ** -24 for k in range(GAIN_DRAWS))


# the clamp together with the step into final_alpha_cumprod == 1 (host test): sampler, eta
CLIP_CASES = (("dpm++2m", 0.0), ("dpm++2m-sde", 0.0), ("ddim", 1.0))

if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    p64 = StableDiffusionPipeline.from_pretrained("tiny", with_decoder=True)
    p64.unet.double(); p64.vae.double()
    emb = embeddings()
    for s, e in SAMPLERS:
        for unc, pred in ((None, "epsilon"), ("u16", "epsilon"), ("u24", "epsilon"), (None, "v_prediction"), ("u16", "v_prediction")):
            if unc == "u24" and (s, e) not in T24_SAMPLERS:
                continue
            seed, g = case_inputs(s, e, unc is not None, pred)
            print(f"{s} eta={e} {pred} uncond={unc} seed {seed} guidance {g}: GAIN "
                  f"{gain(p64, s, e, pred, g, seed, None if unc is None else emb[unc], emb['cond']):.1f}", flush=True)
        for unc in (None, "u16"):
            print(f"{s} eta={e} epsilon uncond={unc} batch seeds {BATCH_SEEDS}: GAIN "
                  + ", ".join(f"{gain(p64, s, e, 'epsilon', GUIDANCE, seed, None if unc is None else emb[unc], emb['cond']):.1f}"
                              for seed in BATCH_SEEDS), flush=True)
    for s, e in CLIP_CASES:
        print(f"{s} eta={e} epsilon unguided, clip_sample and set_alpha_to_one, seed {SINGLE_SEED}: GAIN "
              f"{gain(p64, s, e, 'epsilon', GUIDANCE, SINGLE_SEED, None, emb['cond'], True, True):.1f}", flush=True)
