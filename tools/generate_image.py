#!/usr/bin/env python
"""Render what a learned embedding has learned: sample images from it (ptp_utils.text2image_ldm_stable) and write them out.

    python tools/generate_image.py --model <checkpoint dir | synthetic-sd15 | tiny> --embedding emb.pt --out out/img
                                   [--steps 50] [--seed 0] [--n 1] [--size 512] [--device cuda]

`--embedding`: a tensor [1, T, D] (or [T, D]) saved with torch.save -- what `optimize_embedding` returns.  Image i is sampled from
seed + i and written to `<out>_<i>.png` when PIL imports, else to `<out>_<i>.npy` (uint8 [H, W, 3])."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    ap.add_argument("--embedding", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    import numpy as np
    import torch
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    emb = torch.load(a.embedding, map_location="cpu", weights_only=True)
    if emb.dim() == 2:
        emb = emb[None]
    ldm, controllers, _ = load_ldm(a.device, a.model, decoder=True)
    controller = next(iter(controllers.values()))
    try:
        from PIL import Image
    except ImportError:
        Image = None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for i in range(a.n):
        image, _ = ptp_utils.text2image_ldm_stable(ldm, emb, controller, num_inference_steps=a.steps,
                                                   generator=torch.Generator().manual_seed(a.seed + i), height=a.size, width=a.size)
        path = f"{a.out}_{i}" + (".png" if Image is not None else ".npy")
        if Image is not None:
            Image.fromarray(image[0]).save(path)
        else:
            np.save(path, image[0])
        print(path)


if __name__ == "__main__":
    main()
