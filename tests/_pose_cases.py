"""What tests/test_pose_transfer_host.py and tests/test_pose_transfer_gpu.py share: an independent numpy restatement of the two
energies of include/skp_targets.h, the map / target pairs of the kernel cases, and the pose-guided loop written out on the public
pieces for an fp64 copy of the modules on the host (`text2image_ldm_stable` itself samples in float32).  The whole-call inputs
(embedding, latents, token ids, step count, scale) are those of tests/_keypoint_cases.py."""
from __future__ import annotations

import numpy as np
import torch

import _keypoint_cases as KC

MODES = ("mse", "cosine")
KINDS = ("random", "equal", "orthogonal", "zero map", "zero target")
EXAMPLE_SEED = 17                         # the example image of the whole-call case: the same tiny model, another initial latent


def energy_and_grad_np(M, T, mode):
    """-> (E [B], G [B, K, R, R], mag_G [B, K, R, R], mag_E [B]) in numpy fp64, element by element from include/skp_targets.h; T is
    [B, K, R, R] or [1, K, R, R].  mag_G and mag_E are the magnitudes the roundings of G and E act on: the formulas with every term
    replaced by its absolute value (a degenerate map's E_k = 1 counts 1)."""
    M = np.asarray(M, dtype=np.float64)
    T = np.broadcast_to(np.asarray(T, dtype=np.float64), M.shape)
    B, K, R, _ = M.shape
    if mode == "mse":
        G = 2.0 * (M - T) / (K * R * R)
        mag = np.abs(M) + np.abs(T)
        return ((M - T) ** 2).reshape(B, -1).mean(axis=1), G, 2.0 * mag / (K * R * R), (mag ** 2).reshape(B, -1).mean(axis=1)
    assert mode == "cosine"
    E, Em = np.zeros(B), np.zeros(B)
    G, Gm = np.zeros_like(M), np.zeros_like(M)
    for b in range(B):
        for k in range(K):
            m, t = M[b, k], T[b, k]
            a, c, d = float((m * m).sum()), float((t * t).sum()), float((m * t).sum())
            if a == 0.0 or c == 0.0:
                E[b] += 1.0 / K
                Em[b] += 1.0 / K
                continue
            mh, th, cos = m / np.sqrt(a), t / np.sqrt(c), d / np.sqrt(a * c)
            E[b] += 0.5 * ((mh - th) ** 2).sum() / K
            Em[b] += 0.5 * ((np.abs(mh) + np.abs(th)) ** 2).sum() / K
            G[b, k] = (cos * mh - th) / (K * np.sqrt(a))
            Gm[b, k] = (np.abs(mh) + np.abs(th)) / (K * np.sqrt(a))
    return E, G, Gm, Em


def pair(kind, B, Bt, K, R, scale, gen):
    """Maps M [B, K, R, R] of size `scale` (1 / 77: softmax scale) and targets [Bt, K, R, R], float32 on the host.
    "equal": the target IS the map (of image 0 when it is shared) -- where the cosine energy cancels; "orthogonal": disjoint
    supports, d = 0 exactly; "zero map" / "zero target": map 0 of every image / the last target all zeros (with K = 1 the only one)."""
    M = torch.rand(B, K, R, R, generator=gen) * scale
    T = torch.rand(Bt, K, R, R, generator=gen) * scale
    if kind == "equal":
        T = M[:Bt].clone()
    elif kind == "orthogonal":
        even = torch.arange(R * R).reshape(R, R) % 2 == 0
        M, T = M * even, T * ~even
    elif kind == "zero map":
        M[:, 0] = 0
    elif kind == "zero target":
        T[:, -1] = 0
    else:
        assert kind == "random"
    return M.contiguous(), T.contiguous()


def example_latent():
    return torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(EXAMPLE_SEED))


def example_targets(model):
    """`pose_targets` [1, K, R, R] of an example image that `model` itself sampled from the embedding of tests/_keypoint_cases.py with
    another initial latent (EXAMPLE_SEED), noised with a fixed gaussian: the same call on the GPU tree and on a host tree."""
    from stablekeypoints_amd import ptp_utils
    emb, _, _ = KC.inputs()
    image, _ = ptp_utils.text2image_ldm_stable(model, emb, None, num_inference_steps=KC.STEPS, latent=example_latent(), height=128,
                                               width=128, output_type="float")
    noise = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(EXAMPLE_SEED + 1))
    return ptp_utils.pose_targets(model, image, emb, list(KC.TOKENS), noise=noise.to(image.device))


def pose_loop(model, emb, lat, target_maps, mode, scale, *, steps=KC.STEPS, sampler="ddim", uncond=None, guidance=7.5, normalize=True):
    """The loop of `text2image_ldm_stable(target_maps=...)` written out on `keypoint_energy_grad`, the documented scale and
    `sampler_latent_step`, in the dtype and on the device of `lat` -> (final latents, [E per step], E at the end)."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    plan = SamplerPlan(model.scheduler, sampler, 0.0)
    timesteps, coefs = plan.plan(steps)
    context = [uncond, emb]
    x0_hist = None if sampler == "ddim" else torch.empty_like(lat)
    kw = dict(target_maps=target_maps, target_energy=mode)
    trace = []
    for i, t in enumerate(timesteps):
        pc, pu, E, g = ptp_utils.keypoint_energy_grad(model, lat, context, t, None, list(KC.TOKENS), None, **kw)
        s = torch.full_like(E, scale * coefs[i].sb)
        if normalize:
            s = s / g.pow(2).mean(dim=(1, 2, 3)).sqrt().clamp_min(1e-12)
        trace.append(E)
        with torch.no_grad():
            lat = ptp_utils.sampler_latent_step(model, None, lat, context, t, guidance, plan=plan, coef=coefs[i], x0_hist=x0_hist,
                                                preds=(pc, pu), grad=g, grad_scale=s)
    E_end = ptp_utils.keypoint_energy_grad(model, lat, context, timesteps[-1], None, list(KC.TOKENS), None, **kw)[2]
    return lat, trace, E_end


_host = {}


def host64_model():
    """The reduced-width tree on the host in fp64 (hooked, with its decoder), made once per process."""
    if "model" not in _host:
        from stablekeypoints_amd.optimize_token import load_ldm
        model, _, _ = load_ldm("cpu", "tiny", feature_upsample_res=KC.R, decoder=True)
        model.unet.double()
        model.vae.double()
        _host["model"] = model
    return _host["model"]


def host64_runs(target_maps):
    """The fp64 loops of the whole-call case for `target_maps` [1, K, R, R] (a host tensor; its fp64 copy is used): {(mode, scale):
    (final latents, [E per step], E at the end)} for both modes at keypoint_scale SCALE and 0.  Kept per process for the tensor it
    was first called with."""
    if "runs" not in _host:
        emb, lat, _ = KC.inputs()
        tg = target_maps.detach().double().cpu()
        _host["runs"] = {(mode, s): pose_loop(host64_model(), emb.double(), lat.double(), tg, mode, s) for mode in MODES
                         for s in (KC.SCALE, 0.0)}
        _host["runs_for"] = tg
    assert torch.equal(_host["runs_for"], target_maps.detach().double().cpu())
    return _host["runs"]
