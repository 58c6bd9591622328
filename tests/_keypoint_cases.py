"""What tests/test_keypoint_guidance_host.py and tests/test_keypoint_guidance_gpu.py share: the inputs of the whole-call case, the
definitions of keypoint guidance restated from the reference's own helpers, and the guided loop written out on the public pieces for
an fp64 copy of the modules on the host (`text2image_ldm_stable` itself samples in float32)."""
from __future__ import annotations

import functools

import torch

R = 32                                    # feature_upsample_res of the reduced-width tree in these tests
TOKENS = (2, 7, 11)
TARGETS = (((.25, .25), (.75, .5), (.5, .8)), ((.6, .3), (.2, .7), (.9, .9)))          # image, token -> (row, col)
SIGMA, STEPS, SCALE = 2.0, 4, 2.0


def inputs():
    """-> (embedding [1, 16, 768], latents [2, 4, 16, 16], keypoints [2, 3, 2]): the embedding first, then the latents, from one
    generator seeded with 3."""
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(1, 16, 768, generator=g)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    return emb, lat, torch.tensor(TARGETS)


def energy_and_grad(M, pos, sigma):
    """-> (E [B], G [B, K, R, R], t [B, K, R, R]) of maps M [B, K, R, R] and positions pos [B, K, 2] in the dtype of M, from the
    reference's own helpers: E_b = find_gaussian_loss_at_point(M_b, pos_b[None], sigma) (one point per token), G = dE_b / dM_b by
    autograd through it, t = gaussian_circle(pos_b)."""
    from stablekeypoints_amd.optimize import find_gaussian_loss_at_point
    from stablekeypoints_amd.optimize_token import gaussian_circle
    B, K, r, _ = M.shape
    with torch.enable_grad():
        leaf = M.detach().clone().requires_grad_()
        E = torch.stack([find_gaussian_loss_at_point(leaf[b], pos[b][None].to(M.dtype), sigma=sigma) for b in range(B)])
        G, = torch.autograd.grad(E.sum(), leaf)
    t = torch.stack([gaussian_circle(pos[b].to(M.dtype), size=r, sigma=sigma) for b in range(B)])
    return E.detach(), G, t


def argmax_distance(model, latents, context, t, keypoints, doubled=False):
    """Mean distance, in image fractions, between the targets and the arg-max pixel centres of the K maps of each image at
    timestep `t` -> [n]."""
    from stablekeypoints_amd import ops
    from stablekeypoints_amd._maps import _materialize_host
    from stablekeypoints_amd.ptp_utils import _predict
    model.unet.__dict__["_skp_hook_controller"].reset()
    records, n = [], keypoints.shape[0]
    with torch.no_grad():
        _predict(model, latents, context, t, doubled, records)
        heads = records[0].heads
        qs, ks = [r.q[-n:] for r in records], [r.k if r.k.shape[0] == 1 else r.k[-n:] for r in records]
        if latents.is_cuda:                 # the row-selecting inference maps the package has always had
            M = ops.attn_map_rows(qs, ks, heads, [r.scale for r in records], R, torch.tensor(TOKENS))
        else:                               # (n * heads, R^2, T) per layer -> mean over layers and heads
            M = sum(_materialize_host(q, k, heads, r.scale, R).reshape(n, heads, R * R, -1).mean(dim=1)
                    for r, q, k in zip(records, qs, ks)) / len(records)
            M = M[..., list(TOKENS)].permute(0, 2, 1)
        M = M.reshape(n, len(TOKENS), R * R).double().cpu()
    flat = M.reshape(n, len(TOKENS), -1).argmax(dim=-1)
    at = torch.stack([(flat // R + 0.5) / R, (flat % R + 0.5) / R], dim=-1)
    return (at - keypoints.double()).norm(dim=-1).mean(dim=1)


def guided_loop(model, emb, lat, keypoints, scale, *, steps=STEPS, sampler="ddim", uncond=None, guidance=7.5, normalize=True):
    """The loop of `text2image_ldm_stable(keypoints=...)` written out on `keypoint_energy_grad`, the documented scale and
    `sampler_latent_step`, in the dtype and on the device of `lat` -> (final latents, [E per step], E at the end, arg-max distance
    at the end); the last two on the final latents at the last timestep of the table."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    plan = SamplerPlan(model.scheduler, sampler, 0.0)
    timesteps, coefs = plan.plan(steps)
    context = [uncond, emb]
    x0_hist = None if sampler == "ddim" else torch.empty_like(lat)
    trace = []
    for i, t in enumerate(timesteps):
        pc, pu, E, g = ptp_utils.keypoint_energy_grad(model, lat, context, t, keypoints, list(TOKENS), SIGMA)
        s = torch.full_like(E, scale * coefs[i].sb)
        if normalize:
            s = s / g.pow(2).mean(dim=(1, 2, 3)).sqrt().clamp_min(1e-12)
        trace.append(E)
        with torch.no_grad():
            lat = ptp_utils.sampler_latent_step(model, None, lat, context, t, guidance, plan=plan, coef=coefs[i], x0_hist=x0_hist,
                                                preds=(pc, pu), grad=g, grad_scale=s)
    _, _, E_end, _ = ptp_utils.keypoint_energy_grad(model, lat, context, timesteps[-1], keypoints, list(TOKENS), SIGMA)
    return lat, trace, E_end, argmax_distance(model, lat, context, timesteps[-1], keypoints)


@functools.lru_cache(maxsize=None)
def host64():
    """The reduced-width tree on the host in fp64 (hooked, with its decoder), and the fp64 loops of the whole-call case at
    keypoint_scale SCALE and 0, made once per process and left unchanged."""
    from stablekeypoints_amd.optimize_token import load_ldm
    model, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=R, decoder=True)
    model.unet.double()
    model.vae.double()
    emb, lat, kp = inputs()
    runs = {s: guided_loop(model, emb.double(), lat.double(), kp, s) for s in (SCALE, 0.0)}
    return model, runs
