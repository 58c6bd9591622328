#!/usr/bin/env python
"""Kernel-level A/B of the two stride-2 convolution kernels on the VAE's down-sampling launches (8 rows, pad 0):
the polyphase Winograd F(4x4,2x2) form (csrc/skp_conv_s2w.hip) against the direct form (csrc/skp_conv_s2.hip), plain and with
the statistics epilogue (the form the step launches).

    python tools/conv_s2w_bench.py [--rounds 7] [--iters 10] [--rows 8] [--out profiles/x.md]

Same process, interleaved rounds (direct, wino, direct+stats, wino+stats per round), medians with the min..max spread of the
rounds beside them; the outputs of the two kernels are compared first (max |dy| / max |y|).  A lab build of the library that
multiplies all 100 (position, phase) blocks (-DS2W_ALL_BLOCKS) is timed the same way with SKP_LIB_PATH pointing at it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 512), (256, 256), (512, 128))       # (channels, input size) of the three VAE Downsample2D layers
PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from stablekeypoints_amd import ops
    N, lib = ops.N, ops.N.lib()
    lines = [f"library: {os.path.basename(os.path.dirname(N.LIB_PATH))}/{os.path.basename(N.LIB_PATH)}, rows {a.rows}, "
             f"{a.rounds} interleaved rounds x {a.iters} launches, median us (min..max of the rounds)", "",
             "| launch | direct | wino | direct + stats | wino + stats | wino / direct (stats) | max abs dy / max abs y | wino + stats, of peak on direct FLOPs |",
             "|---|---|---|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    for C, sz in SHAPES:
        B = a.rows
        x = torch.randn(B, C, sz, sz, generator=g).cuda()
        w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).cuda()
        bias = torch.randn(C, generator=g).cuda()
        Ud = torch.empty(9 * C * C, device="cuda")
        Uw = torch.empty(100 * C * C, device="cuda")            # 81 blocks per channel group (100 in the all-blocks lab build)
        N.check(lib.skp_conv3x3_s2_filter_f32(w.data_ptr(), Ud.data_ptr(), C, C, ops._stream()), "filter")
        N.check(lib.skp_conv3x3_s2w_filter_f32(w.data_ptr(), Uw.data_ptr(), C, C, 0, ops._stream()), "filter w")
        yd = torch.empty(B, C, sz // 2, sz // 2, device="cuda")
        yw = torch.empty_like(yd)
        sd = torch.empty(B, C, (sz // 16) * (sz // 32), 2, device="cuda")
        sw = torch.empty(B, C, (sz // 8) * (sz // 8) // 16, 2, device="cuda")
        st = ops._stream()
        args = (B, C, C, sz, sz, 0, st)
        fns = {
            "direct": lambda: N.check(lib.skp_conv3x3_s2_f32(x.data_ptr(), Ud.data_ptr(), bias.data_ptr(), yd.data_ptr(), *args), "d"),
            "wino": lambda: N.check(lib.skp_conv3x3_s2w_f32(x.data_ptr(), Uw.data_ptr(), bias.data_ptr(), yw.data_ptr(), *args), "w"),
            "direct_stats": lambda: N.check(lib.skp_conv3x3_s2_stats_f32(x.data_ptr(), Ud.data_ptr(), bias.data_ptr(), yd.data_ptr(),
                                                                         sd.data_ptr(), *args), "ds"),
            "wino_stats": lambda: N.check(lib.skp_conv3x3_s2w_stats_f32(x.data_ptr(), Uw.data_ptr(), bias.data_ptr(), yw.data_ptr(),
                                                                        sw.data_ptr(), *args), "ws"),
        }
        for f in fns.values():
            f(); f()
        torch.cuda.synchronize()
        err = ((yw - yd).abs().max() / yd.abs().max()).item()
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
        med = {k: statistics.median(v) for k, v in times.items()}
        cell = lambda k: f"{med[k]:.0f} ({min(times[k]):.0f}..{max(times[k]):.0f})"
        flops = 2.0 * 9 * C * C * B * (sz // 2) ** 2
        lines.append(f"| {C}->{C} @{sz}^2 | {cell('direct')} | {cell('wino')} | {cell('direct_stats')} | {cell('wino_stats')} | "
                     f"{med['wino_stats'] / med['direct_stats']:.3f} | {err:.2e} | {flops / med['wino_stats'] / 1e6 / PEAK_TF:.2f} |")
        del x, w, Ud, Uw, yd, yw
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
