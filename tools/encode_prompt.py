#!/usr/bin/env python
"""Turn a prompt into an embedding file: the context the UNet's cross-attention layers take, from the checkpoint's own tokenizer and
text encoder (ptp_utils.encode_prompt).

    python tools/encode_prompt.py --model <checkpoint dir | synthetic-sd15 | tiny> --prompt "a photo of a cat" --out emb.pt
                                  [--device cuda]

Writes a float32 tensor [1, 77, D] with torch.save: what `tools/generate_image.py --embedding` and `--uncond` load (`--prompt ""`
gives the unconditional embedding CLIP("")).  SDXL: the 2048-channel context; the pooled vector goes to `<out>.pooled.pt`."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    ap.add_argument("--prompt", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    import torch
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, _, _ = load_ldm(a.device, a.model, text_encoder=True)
    emb = ptp_utils.encode_prompt(ldm, [a.prompt])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if isinstance(emb, tuple):
        torch.save(emb[1].float().cpu(), a.out + ".pooled.pt")
        emb = emb[0]
    torch.save(emb.float().cpu(), a.out)
    print(a.out, tuple(emb.shape))


if __name__ == "__main__":
    main()
