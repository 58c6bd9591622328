#!/usr/bin/env python
"""Informational timing of the text encoder (profiles/text_encoder.md): one prompt through a tower on the causal kernel route and
under ops.TEXT_ATTN_MODE = "lib", in alternating windows of one process; plus the routes table of one encode and the tower's size.

    python tools/text_encoder_bench.py [--model sd15] [--windows 5] [--reps 200] [--warmup 10] [--out result.json]

A window is `--warmup` untimed and `--reps` timed `ptp_utils.encode_prompt` calls (tokenising included) under a host clock that stops
after a device synchronise.  Needs the GPU; prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd15")
    ap.add_argument("--prompt", default="a photo of a cat")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from stablekeypoints_amd import ops, ptp_utils, routes
    from stablekeypoints_amd.ldm.clip import n_params
    from stablekeypoints_amd.optimize_token import load_ldm
    assert torch.cuda.is_available(), "text_encoder_bench needs the MI355X"
    ldm, _, _ = load_ldm("cuda", a.model, feature_upsample_res=128, text_encoder=True)
    out = {"model": a.model, "parameters": n_params(ldm.text_encoder)}

    def encode():
        e = ptp_utils.encode_prompt(ldm, [a.prompt])
        return e[0] if isinstance(e, tuple) else e
    routes.reset()
    encode()
    torch.cuda.synchronize()
    out["routes_table"] = routes.table()

    def window(mode):
        ops.TEXT_ATTN_MODE = mode
        for _ in range(a.warmup):
            encode()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            encode()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.reps * 1e3
    ms = {"auto": [], "lib": []}
    for _ in range(a.windows):
        for mode in ms:
            ms[mode].append(window(mode))
    out["ms_per_encode"] = ms
    ops.TEXT_ATTN_MODE = "auto"
    x = encode()
    ops.TEXT_ATTN_MODE = "lib"
    y = encode()
    ops.TEXT_ATTN_MODE = "auto"
    out["auto_vs_lib_max_abs"], out["out_abs_max"] = float((x - y).abs().max()), float(x.abs().max())
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
