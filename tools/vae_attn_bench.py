#!/usr/bin/env python3
"""VAE mid-block attention core (one head of d = 512): the wide flash kernel against the library route on the same tensors.

    python tools/vae_attn_bench.py --out profiles/vae_attention.md

Both routes compute softmax(q k^T / sqrt(512)) v for q, k, v [rows, keys, 512]:
    flash_wide   ops.flash_attn_wide (csrc/skp_flash_attn_wide.hip)
    lib_core     baddbmm + softmax + bmm, as ldm/fused.py::_vae_attention_forward runs it
One process; per shape the two routes alternate over ROUNDS rounds, each round one window of `reps` calls between two device
events, `reps` chosen so that a window lasts about WINDOW seconds.  Reported per route: the median window (ms per call), the
run-to-run spread (max - min over the median), the peak allocation over one call; and flash / lib, the kernel's FLOP rate
(4 rows keys^2 512 FLOP per call) and its share of the fp32 matrix peak.  Needs the GPU: there is no CPU path."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8, 4096), (2, 4096), (1, 4096), (1, 9216), (2, 9216), (1, 16384), (2, 16384)]      # (rows, keys)
D = 512
PEAK_F32_MATRIX_TFLOPS = 157.3           # MI355X fp32 MFMA, dense
ROUNDS = 5
WINDOW = 0.3


def lib_core(q, k, v, scale):
    attn = torch.baddbmm(torch.empty(q.shape[0], q.shape[1], k.shape[1], dtype=q.dtype, device=q.device),
                         q, k.transpose(1, 2), beta=0, alpha=scale).softmax(dim=-1)
    return torch.bmm(attn, v)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def measure(rows, keys, ops):
    g = torch.Generator(device="cuda").manual_seed(rows * 100003 + keys)
    q, k, v = (torch.randn(rows, keys, D, device="cuda", generator=g) for _ in range(3))
    scale = D ** -0.5
    fns = {"flash_wide": lambda: ops.flash_attn_wide(q, k, v, 1, scale), "lib_core": lambda: lib_core(q, k, v, scale)}
    res = {}
    for name, fn in fns.items():                               # warm-up, agreement, repeat count
        y = fn()
        res[name] = {"out": y}
        for _ in range(2):
            fn()
        once = window_ms(fn, 3)
        res[name]["reps"] = max(3, min(400, int(WINDOW * 1e3 / once)))
        res[name]["peak_bytes"] = peak_bytes(fn)
        res[name]["windows_ms"] = []
    diff = (res["flash_wide"]["out"] - res["lib_core"]["out"]).abs().max().item() / res["lib_core"]["out"].abs().max().item()
    for name in fns:
        del res[name]["out"]
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            res[name]["windows_ms"].append(window_ms(fn, res[name]["reps"]))
    row = {"rows": rows, "keys": keys, "max_rel_diff": diff, "flop": 4.0 * rows * keys * keys * D}
    for name in fns:
        w = res[name]["windows_ms"]
        med = statistics.median(w)
        row[name] = {"ms": med, "spread": (max(w) - min(w)) / med, "windows_ms": w, "reps": res[name]["reps"],
                     "peak_bytes": res[name]["peak_bytes"]}
    row["ratio"] = row["flash_wide"]["ms"] / row["lib_core"]["ms"]
    row["flash_tflops"] = row["flop"] / (row["flash_wide"]["ms"] * 1e-3) / 1e12
    row["share_of_peak"] = row["flash_tflops"] / PEAK_F32_MATRIX_TFLOPS
    del q, k, v
    torch.cuda.empty_cache()
    return row


def gate(results):
    """The rule of the automatic route above 8 192 keys: open if flash_wide is no slower than lib_core by more than the measured
    spread at every shape with more than 8 192 keys."""
    big = [r for r in results if r["keys"] > 8192]
    verdict = []
    for r in big:
        slack = max(r["flash_wide"]["spread"], r["lib_core"]["spread"])
        verdict.append((r["rows"], r["keys"], r["ratio"], slack, r["ratio"] <= 1.0 + slack))
    return verdict


def markdown(results, device):
    lines = ["# VAE mid-block attention core: `flash_wide` against `lib_core`", "",
             f"Measured by `tools/vae_attn_bench.py` on {device}; every number below is from that run.  q, k, v `[rows, keys, 512]`"
             " fp32 random normal, scale 512^-1/2; one process, the two routes alternating over "
             f"{ROUNDS} rounds, one window of `reps` calls between device events per round (about {WINDOW} s each); ms = median"
             " window per call, spread = (max - min) / median over the rounds, peak = largest allocation over one call beyond"
             " the inputs, rate = 4 rows keys^2 512 FLOP over the flash time, share = rate over the"
             f" {PEAK_F32_MATRIX_TFLOPS} TFLOP/s fp32 matrix peak.  `lib_core` = `baddbmm` + `softmax` + `bmm`.", "",
             "| rows | keys | flash_wide ms | spread | lib_core ms | spread | flash / lib | flash peak MiB | lib peak MiB | "
             "flash TFLOP/s | share of peak | max rel. difference |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        f, l = r["flash_wide"], r["lib_core"]
        lines.append(f"| {r['rows']} | {r['keys']} | {f['ms']:.3f} | {100 * f['spread']:.1f} % | {l['ms']:.3f} | "
                     f"{100 * l['spread']:.1f} % | {r['ratio']:.2f} | {f['peak_bytes'] / 2**20:.1f} | {l['peak_bytes'] / 2**20:.1f} | "
                     f"{r['flash_tflops']:.1f} | {100 * r['share_of_peak']:.0f} % | {r['max_rel_diff']:.1e} |")
    lines += ["", "## The automatic route above 8 192 keys", "",
              "Rule: the gate opens if `flash_wide` is no slower than `lib_core` by more than the measured spread at the 9 216- and"
              " 16 384-key shapes; otherwise `ops.VAE_FLASH_MIN_KEYS` is set so that `\"auto\"` opens only where `lib_core`'s two"
              " score matrices exceed 8 GiB.", "",
              "| rows | keys | flash / lib | larger spread | within the spread |", "|---|---|---|---|---|"]
    v = gate(results)
    for rows, keys, ratio, slack, ok in v:
        lines.append(f"| {rows} | {keys} | {ratio:.2f} | {100 * slack:.1f} % | {'yes' if ok else 'no'} |")
    lines += ["", "Verdict of this run: " + ("the gate opens at 8 192 keys." if v and all(x[4] for x in v) else
                                              "`flash_wide` is slower; the route exists for memory, not speed."), ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the markdown table here (default: print only)")
    ap.add_argument("--json", default=None, help="write the raw windows here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/vae_attn_bench.py needs the GPU: timings from a CPU say nothing about the kernel")
    from stablekeypoints_amd import ops
    ops.N.lib()
    results = []
    for rows, keys in SHAPES:
        r = measure(rows, keys, ops)
        results.append(r)
        print(f"rows {rows} keys {keys}: flash_wide {r['flash_wide']['ms']:.3f} ms (+-{100 * r['flash_wide']['spread']:.1f} %), "
              f"lib_core {r['lib_core']['ms']:.3f} ms (+-{100 * r['lib_core']['spread']:.1f} %), flash / lib {r['ratio']:.2f}, "
              f"{r['flash_tflops']:.1f} TFLOP/s, diff {r['max_rel_diff']:.1e}", flush=True)
    md = markdown(results, torch.cuda.get_device_name(0))
    print(md)
    for path, text in ((a.out, md), (a.json, json.dumps(results, indent=1))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
