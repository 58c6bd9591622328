#!/usr/bin/env python
"""Time image sampling (ptp_utils.text2image_ldm_stable): single-image calls against one batched call, with and without
classifier-free guidance, and print the route table of one guided step.

    python tools/generate_bench.py [--model synthetic-sd15] [--size 512] [--steps 10] [--n 4] [--rounds 3] [--tokens 77] [--json FILE]
                                   [--sampler ddim|dpm++2m|dpm++2m-sde [--eta 0] [--sampler-steps K]] [--variants A,G1] [--keypoints]
                                   [--pose] [--capture]

Every timed call ends in a device synchronise (the uint8 image is copied to the host); every shape is warmed up once before the
timed rounds; the variants run alternately inside each round, so a drift of the machine shows up as spread, not as a difference.
  A  n single-image calls, unguided (what tools/generate_image.py does without --batch)
  B  one call with n images, unguided
  G1 / Gn      guided (uncond and cond of equal length: one UNet forward of 2 / 2n rows per step), 1 image / n images
  G1_two       guided, 1 image, uncond one token shorter than cond: two forwards of 1 row per step
`--sampler NAME`: every variant is timed a second time as `<variant>@NAME/K`, sampled by NAME in K = `--sampler-steps` steps (default:
`--steps`), in turn with the default call at `--steps` -- e.g. `--steps 50 --sampler dpm++2m --sampler-steps 20 --n 1 --variants A,G1`
times the 20-step DPM-Solver++ image against the 50-step DDIM image, unguided and guided.  `--variants`: only these.
`--keypoints`: every variant is timed a second time as `<variant>+kp`, the same call with keypoint guidance (K = 10 tokens, targets
drawn from the seed, every step guided), in turn with the call without it (with `--sampler` also `<variant>@NAME/K+kp`); and `ops.MapPointLossFn` (forward and backward) is
timed against the route the package had before it -- dense fused maps under autograd, a gather, torch ops for the target and the
MSE -- on the hooked layers of SD-1.5 at 512^2 (sides 16, 16, 16, 32; 8 heads of 160, 160, 160, 80 channels; R = 128) with
T = 77 and T = 500 tokens, K = 10, n = 1 and 4 rows.
`--pose`: every variant is timed as `<variant>+kp` (as with `--keypoints`) and, in turn with it, as `<variant>+pose` and
`<variant>+pose-mse`: the same call guided toward target MAPS (`target_maps=`, the cosine and the mse energy) -- the maps
`ptp_utils.pose_targets` takes from a random image for the same K = 10 tokens, one target for every image -- so the pose-guided
call stands next to the point-guided call of the same shape; and the energy kernels alone, `ops.map_target_loss` (both modes)
against `ops.point_loss`, at K = 10, R = 128 with 1 and 4 rows and at K = 3, R = 32 with 2 rows.
`--capture`: every variant (those of the other flags included) is timed a second time as `<variant>+graph`, the same call with
`capture=True` -- two steps on eager launches, the rest as replays of one recorded step -- in turn with the eager call; the
warm-up call of each variant is timed too and printed as `first call`: for a `+graph` variant it holds the one-off cost of
recording (a dry run of the step, the capture, the graph's instantiation), which later calls with the same key do not pay.
Times are per image."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic-sd15")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--json", default=None)
    ap.add_argument("--sampler", default=None, choices=("ddim", "dpm++2m", "dpm++2m-sde"))
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--sampler-steps", type=int, default=None)
    ap.add_argument("--variants", default=None)
    ap.add_argument("--keypoints", action="store_true")
    ap.add_argument("--pose", action="store_true")
    ap.add_argument("--capture", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "generate_bench.py measures the GPU path only"
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cuda", a.model, decoder=True, init_on_device=True)
    ctrl = next(iter(controllers.values()))
    dim = int(ldm.unet.config["cross_attention_dim"]) if hasattr(ldm.unet, "config") else 768
    g = torch.Generator().manual_seed(0)
    cond = torch.randn(1, a.tokens, dim, generator=g)
    unc = torch.randn(1, a.tokens, dim, generator=g)
    kw = dict(num_inference_steps=a.steps, height=a.size, width=a.size)

    def gens(first, count):
        return [torch.Generator().manual_seed(first + i) for i in range(count)]

    def single(**extra):
        for gen in gens(0, a.n):
            ptp_utils.text2image_ldm_stable(ldm, cond, ctrl, generator=gen, **{**kw, **extra})
        return a.n

    def batched(count, **extra):
        ptp_utils.text2image_ldm_stable(ldm, cond, ctrl, generator=gens(0, count), **{**kw, **extra})
        return count
    guide = dict(uncond_embedding=unc, guidance_scale=7.5)

    def make(**over):
        """The variants, with `over` on top of every call's keywords."""
        return {
            "A": lambda: single(**over),
            "B": lambda: batched(a.n, **over),
            "G1": lambda: batched(1, **guide, **over),
            "Gn": lambda: batched(a.n, **guide, **over),
            "G1_two": lambda: batched(1, uncond_embedding=unc[:, :-1], guidance_scale=7.5, **over),
        }
    variants = make()
    names = a.variants.split(",") if a.variants else list(variants)
    unknown = [k for k in names if k not in variants]
    if unknown or not names:
        ap.error(f"--variants: unknown {unknown}; choose from {list(variants)}")
    overs = {"": {}}                                            # name suffix -> keywords on top of every call's; the two flags compose
    if a.sampler is not None:
        k_steps = a.sampler_steps or a.steps
        overs[f"@{a.sampler}/{k_steps}"] = dict(sampler=a.sampler, eta=a.eta, num_inference_steps=k_steps)
    if a.keypoints or a.pose:
        kp_ids = torch.randperm(a.tokens, generator=g)[:10].sort().values
        kp = dict(keypoints=torch.rand(len(kp_ids), 2, generator=g), keypoint_indices=kp_ids)
        guided = [("+kp", kp)]
        if a.pose:
            example = torch.rand(1, 3, a.size, a.size, generator=g)
            maps = ptp_utils.pose_targets(ldm, example, cond, kp_ids)
            guided += [("+pose", dict(target_maps=maps, target_energy="cosine", keypoint_indices=kp_ids)),
                       ("+pose-mse", dict(target_maps=maps, target_energy="mse", keypoint_indices=kp_ids))]
        overs = {name: o for suffix, over in overs.items()
                 for name, o in [(suffix, over)] + [(suffix + tail, {**over, **extra}) for tail, extra in guided]}
    if a.capture:
        overs = {name: o for suffix, over in overs.items() for name, o in ((suffix, over), (suffix + "+graph", {**over, "capture": True}))}
    made = {suffix: make(**over) for suffix, over in overs.items()}
    variants = {k + suffix: made[suffix][k] for k in names for suffix in overs}
    width = max([7] + [len(k) for k in variants])
    times = {k: [] for k in variants}
    first = {}
    for k, fn in variants.items():                              # warm-up: every shape once (a +graph variant records its step here)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        first[k] = time.perf_counter() - t0
    for _ in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            images = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / images)
    print(f"{a.model} at {a.size}^2, {a.steps} steps, n = {a.n}, {a.tokens} tokens, {a.rounds} rounds; seconds per image")
    for k, ts in times.items():
        print(f"  {k:{width}s} median {sorted(ts)[len(ts) // 2]:.4f}   min {min(ts):.4f}   max {max(ts):.4f}   all {[round(t, 4) for t in ts]}")
    if a.capture:
        print("first call of each variant, seconds for the whole call (all its images; caches, library choices and, for +graph, the "
              "recording):\n  " + "   ".join(f"{k} {v:.3f}" for k, v in first.items()))
        cache = ptp_utils.sample_graphs(ldm)
        print(f"recorded steps kept on the model: {len(cache.keys())} keys, {cache.hits} hits, {cache.misses} misses")
    # routes of ONE guided step (2 rows) and of one guided step of n images (2n rows)
    tables = {}
    t = ldm.scheduler.timesteps[0]
    for rows in (1, a.n):
        lat = torch.randn(2 * rows, 4, a.size // 8, a.size // 8, device="cuda")
        before = routes.snapshot()
        with torch.no_grad(), ptp_utils.ops.up2_in_unet():
            ptp_utils.guided_latent_step(ldm, ctrl, lat, [unc.cuda(), cond.cuda()], t, 7.5, doubled=True)
        ctrl.reset()
        tables[2 * rows] = routes.table(routes.delta(before))
        print(f"\nroutes of one guided step, {2 * rows} rows per forward:\n{tables[2 * rows]}")
    node = node_against_older_route(a.rounds) if a.keypoints else {}
    energy = target_loss_against_point_loss(a.rounds) if a.pose else {}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(args=vars(a), seconds_per_image=times, first_call_seconds=first, routes={str(k): v for k, v in tables.items()},
                           map_point_loss_seconds=node, energy_kernel_seconds=energy), f, indent=1)


def target_loss_against_point_loss(rounds, calls=200):
    """`ops.map_target_loss` (mse, cosine; a shared target) against `ops.point_loss` on random maps of softmax scale; `calls` of each
    per timed window, the three in turn; -> {shape: {kernel: [seconds per call]}}."""
    import torch
    from stablekeypoints_amd import ops
    out = {}
    for B, K, R in ((1, 10, 128), (4, 10, 128), (2, 3, 32)):
        g = torch.Generator().manual_seed(B + K + R)
        M = (torch.rand(B, K, R, R, generator=g) / 77).cuda()
        T = (torch.rand(1, K, R, R, generator=g) / 77).cuda()
        pos = torch.rand(B, K, 2, generator=g).cuda()
        fns = {"point_loss": lambda: ops.point_loss(M, pos, 2.0), "map_target_loss mse": lambda: ops.map_target_loss(M, T, "mse"),
               "map_target_loss cosine": lambda: ops.map_target_loss(M, T, "cosine")}
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        for _ in range(rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / calls)
        out[f"B={B} K={K} R={R}"] = times
        print(f"energy and unit gradient, B = {B}, K = {K}, R = {R}: " + ", ".join(
            f"{k} median {sorted(ts)[len(ts) // 2] * 1e6:.1f} us (min {min(ts) * 1e6:.1f})" for k, ts in times.items()))
    return out


def node_against_older_route(rounds, K=10, R=128, sides=(16, 16, 16, 32), heads=8, widths=(1280, 1280, 1280, 640), calls=20):
    """Forward + backward (dq) of `ops.MapPointLossFn` against dense `fused_maps` + gather + torch MSE under autograd, on random
    q / k of the hooked SD-1.5 layers at 512^2; `calls` of each per timed window, the two in turn; -> {shape: {route: [seconds per
    call]}}."""
    import torch
    from stablekeypoints_amd import ops
    from stablekeypoints_amd._maps import FusedAttn, fused_maps
    from stablekeypoints_amd.optimize_token import gaussian_circle
    out = {}
    for T, n in ((77, 1), (77, 4), (500, 1), (500, 4)):
        g = torch.Generator().manual_seed(T + n)
        qs = [torch.randn(n, s * s, c, generator=g).cuda().requires_grad_() for s, c in zip(sides, widths)]
        ks = [torch.randn(1, T, c, generator=g).cuda() for c in widths]
        scales = [(c // heads) ** -0.5 for c in widths]
        ids = torch.randperm(T, generator=g)[:K].sort().values
        pos = torch.rand(n, K, 2, generator=g).cuda()
        tokrow = torch.full((T,), -1, dtype=torch.int32)
        tokrow[ids] = torch.arange(K, dtype=torch.int32)
        meta = dict(R=R, heads=heads, scales=scales, sigma=2.0, pos=pos, sel=ids.cuda(), tokrow=tokrow.cuda())
        flat = [v for q, k in zip(qs, ks) for v in (q, k)]

        def node():
            torch.autograd.grad(ops.MapPointLossFn.apply(meta, *flat).sum(), qs)

        def older():
            M = fused_maps([FusedAttn(q, k, heads, sc, R) for q, k, sc in zip(qs, ks, scales)])[:, meta["sel"]]
            t = torch.stack([gaussian_circle(pos[b], size=R, sigma=2.0) for b in range(n)])
            torch.autograd.grad(((M - t) ** 2).mean(dim=(1, 2, 3)).sum(), qs)
        fns = {"map_point_loss": node, "older_route": older}
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        for _ in range(rounds):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / calls)
        out[f"T={T} n={n}"] = times
        print(f"map + point loss, forward and backward, T = {T}, n = {n}: " + ", ".join(
            f"{k} median {sorted(ts)[len(ts) // 2] * 1e3:.3f} ms (min {min(ts) * 1e3:.3f})" for k, ts in times.items()))
    return out


if __name__ == "__main__":
    main()
