#!/usr/bin/env python
"""Time image sampling (ptp_utils.text2image_ldm_stable): single-image calls against one batched call, with and without
classifier-free guidance, and print the route table of one guided step.

    python tools/generate_bench.py [--model synthetic-sd15] [--size 512] [--steps 10] [--n 4] [--rounds 3] [--tokens 77] [--json FILE]
                                   [--sampler ddim|dpm++2m|dpm++2m-sde [--eta 0] [--sampler-steps K]] [--variants A,G1]

Every timed call ends in a device synchronise (the uint8 image is copied to the host); every shape is warmed up once before the
timed rounds; the variants run alternately inside each round, so a drift of the machine shows up as spread, not as a difference.
  A  n single-image calls, unguided (what tools/generate_image.py does without --batch)
  B  one call with n images, unguided
  G1 / Gn      guided (uncond and cond of equal length: one UNet forward of 2 / 2n rows per step), 1 image / n images
  G1_two       guided, 1 image, uncond one token shorter than cond: two forwards of 1 row per step
`--sampler NAME`: every variant is timed a second time as `<variant>@NAME/K`, sampled by NAME in K = `--sampler-steps` steps (default:
`--steps`), in turn with the default call at `--steps` -- e.g. `--steps 50 --sampler dpm++2m --sampler-steps 20 --n 1 --variants A,G1`
times the 20-step DPM-Solver++ image against the 50-step DDIM image, unguided and guided.  `--variants`: only these.
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
    variants = {k: variants[k] for k in names}
    if a.sampler is not None:
        k_steps = a.sampler_steps or a.steps
        named = make(sampler=a.sampler, eta=a.eta, num_inference_steps=k_steps)
        variants = {name: fn for k in names for name, fn in ((k, variants[k]), (f"{k}@{a.sampler}/{k_steps}", named[k]))}
    width = max([7] + [len(k) for k in variants])
    times = {k: [] for k in variants}
    for k, fn in variants.items():                              # warm-up: every shape once
        fn()
    torch.cuda.synchronize()
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
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(args=vars(a), seconds_per_image=times, routes={str(k): v for k, v in tables.items()}), f, indent=1)


if __name__ == "__main__":
    main()
