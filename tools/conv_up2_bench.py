#!/usr/bin/env python
"""Kernel-level A/B of the two routes of an Upsample2D (nearest 2x + 3x3 convolution) at the VAE decoder's and the UNet's launch
shapes, one image: the polyphase kernel on the low-resolution input (csrc/skp_conv_up2.hip) against F.interpolate +
ops.conv3x3_auto on the up-sampled tensor (the Winograd kernels).

    python tools/conv_up2_bench.py [--rounds 7] [--iters 10] [--rows 1] [--decode] [--sample STEPS] [--out profiles/x.md]

Same process, interleaved rounds, medians with the min..max spread of the rounds beside them; the two outputs are compared first.
`--decode`: one full-width (`sd15`, seeded synthetic weights) 512^2 decode; `--sample STEPS`: one STEPS-step 512^2 sample, both
with the library's own gate."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, low-resolution size): the decoder's three up-samplers at 512^2, then the UNet's three
SHAPES = ((512, 64), (512, 128), (256, 256), (1280, 8), (1280, 16), (640, 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--sample", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from stablekeypoints_amd import ops
    N = ops.N
    N.lib()
    F = torch.nn.functional
    lines = [f"rows {a.rows}, {a.rounds} interleaved rounds x {a.iters} launches, median us (min..max of the rounds)", "",
             "| launch (low-res) | interpolate + conv3x3_auto | up2_poly | up2 / interp | max abs dy / max abs y |", "|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for C, sz in SHAPES:
            B = a.rows
            x = torch.randn(B, C, sz, sz, generator=g).cuda()
            w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).cuda()
            bias = torch.randn(C, generator=g).cuda()

            def interp():
                return ops.conv3x3_auto(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, bias)

            def up2():
                return ops.conv3x3_up2(x, w, bias)
            fns = {"interp": interp, "up2": up2}
            N.tune("conv_up2", 1)
            try:
                for f in fns.values():
                    f(); f()
                torch.cuda.synchronize()
                ya, yb = interp(), up2()
                err = ((ya - yb).abs().max() / ya.abs().max()).item()
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k, f in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            f()
                        e1.record()
                        torch.cuda.synchronize()
                        times[k].append(e0.elapsed_time(e1) / a.iters * 1e3)
            finally:
                N.tune("conv_up2", 0)
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = lambda k: f"{med[k]:.0f} ({min(times[k]):.0f}..{max(times[k]):.0f})"
            lines.append(f"| {C}->{C} @{sz}^2 | {cell('interp')} | {cell('up2')} | {med['up2'] / med['interp']:.3f} | {err:.2e} |")
            del x, w, bias, ya, yb
        if a.decode or a.sample:
            from stablekeypoints_amd import ptp_utils
            from stablekeypoints_amd.optimize_token import load_ldm
            ldm, controllers, _ = load_ldm("cuda", "sd15", feature_upsample_res=128, init_on_device=True, decoder=True)
            ctrl = next(iter(controllers.values()))
            z = torch.randn(1, 4, 64, 64, generator=g).cuda()
            if a.decode:
                ts = []
                for _ in range(4):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    ldm.vae.decode(z, to_image=True)
                    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                lines += ["", f"sd15 512^2 decode (one image, 4 calls, ms): {', '.join(f'{t:.1f}' for t in ts)}"]
            if a.sample:
                emb = torch.randn(1, 77, 768, generator=g).cuda()
                ts = []
                for _ in range(2):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, num_inference_steps=a.sample, generator=torch.Generator().manual_seed(0))
                    torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
                lines += ["", f"sd15 512^2 sample, {a.sample} steps (2 calls, s): {', '.join(f'{t:.2f}' for t in ts)}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
