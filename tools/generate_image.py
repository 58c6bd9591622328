#!/usr/bin/env python
"""Render what a learned embedding has learned: sample images from it (ptp_utils.text2image_ldm_stable) and write them out.

    python tools/generate_image.py --model <checkpoint dir | synthetic-sd15 | tiny> (--embedding emb.pt | --prompt TEXT) --out out/img
                                   [--steps 50] [--seed 0] [--n 1] [--size 512] [--device cuda]
                                   [--uncond unc.pt | --negative-prompt TEXT] [--guidance 7.5] [--batch 1] [--prediction-type epsilon|v_prediction|sample]
                                   [--sampler ddim|dpm++2m|dpm++2m-sde] [--eta 0]
                                   [--keypoints "r,c;r,c;..."|FILE.pt --keypoint-indices FILE.pt|"i,j,..." [--keypoint-scale 2]
                                    [--keypoint-sigma 2] [--keypoint-steps 0,1]] [--capture]
                                   [--pose-from IMAGE --keypoint-indices FILE.pt|"i,j,..." [--pose-energy cosine|mse]
                                    [--pose-noise-level -1] [--keypoint-scale 2] [--keypoint-steps 0,1]]

`--embedding`: a tensor [1, T, D] (or [T, D]) saved with torch.save -- what `optimize_embedding` returns.  Image i is sampled from
seed + i and written to `<out>_<i>.png` when PIL imports, else to `<out>_<i>.npy` (uint8 [H, W, 3]).
`--uncond`: a tensor saved the same way, the unconditional / negative embedding of classifier-free guidance with strength
`--guidance` (its token count may differ from the embedding's); without it only the embedding conditions the UNet.
`--prompt TEXT`: sample from a plain prompt through the checkpoint's text encoder instead of a learned embedding;
`--negative-prompt TEXT`: the unconditional side as a prompt (the empty string is valid and means CLIP("")).  Either one loads the
text encoder and its tokenizer with the model (tools/encode_prompt.py writes the same embeddings to files).
`--batch B`: B images per sampling call (the seeds, the images' starting noise and the file names do not depend on it).
`--prediction-type`: what the UNet predicts; default: the checkpoint's scheduler/scheduler_config.json, else epsilon.
`--sampler`: ddim (the default), dpm++2m (DPM-Solver++ 2M: try `--steps 20`) or dpm++2m-sde; `--eta` in (0, 1] adds DDIM's variance
noise (it selects ddim when `--sampler` is not given, and is an error with another sampler);
the stochastic ones draw their noise from the image's seed, after its starting noise, so an image does not depend on `--batch`.
`--keypoints` with `--keypoint-indices`: keypoint guidance -- K target positions (row, col) in image fractions, written out or a
tensor [K, 2] saved with torch.save (the same targets for every image), for K token ids of the embedding, written out or the
tensor `find_best_indices` returned (the reference's outputs/indices.pt); `--keypoint-scale`, `--keypoint-sigma` (map pixels) and
`--keypoint-steps lo,hi` (the guided fraction of the steps) as in `text2image_ldm_stable`.  Prints each image's energy at the first
and at the last guided step.  The default scale was only tried on the seeded reduced-width tree, never on trained weights.
`--pose-from IMAGE` with `--keypoint-indices` (not together with `--keypoints`): pose transfer -- the image is loaded through
`CustomDataset`'s resize at `--size`, `ptp_utils.pose_targets` takes the attention maps of the K tokens on it (noised to
`--pose-noise-level`, an index into the scheduler's timestep table; the noise is drawn from `--seed`), and every image is guided
toward those maps with `--pose-energy` (cosine, the default, or mse), `--keypoint-scale` and `--keypoint-steps`.  The default scale was,
for either energy, only tried on the seeded reduced-width tree.
`--capture` (off by default): `text2image_ldm_stable(capture=True)` -- after two steps on eager launches the rest of every call
replays one recorded step; the images are the same, bit for bit, and calls after the first reuse the recording."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    ap.add_argument("--embedding", default=None)
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--negative-prompt", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--uncond", default=None)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prediction-type", default=None, choices=("epsilon", "v_prediction", "sample"))
    ap.add_argument("--sampler", default=None, choices=("ddim", "dpm++2m", "dpm++2m-sde"))
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--keypoints", default=None)
    ap.add_argument("--keypoint-indices", default=None)
    ap.add_argument("--keypoint-scale", type=float, default=2.0)
    ap.add_argument("--keypoint-sigma", type=float, default=2.0)
    ap.add_argument("--keypoint-steps", default="0,1")
    ap.add_argument("--capture", action="store_true")
    ap.add_argument("--pose-from", default=None)
    ap.add_argument("--pose-energy", default="cosine", choices=("cosine", "mse"))
    ap.add_argument("--pose-noise-level", type=int, default=-1)
    a = ap.parse_args()
    import numpy as np
    import torch
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.optimize_token import load_ldm
    if (a.embedding is None) == (a.prompt is None):
        ap.error("exactly one of --embedding and --prompt")
    if a.uncond is not None and a.negative_prompt is not None:
        ap.error("--uncond and --negative-prompt are mutually exclusive")
    emb = None
    if a.embedding is not None:
        emb = torch.load(a.embedding, map_location="cpu", weights_only=True)
        if emb.dim() == 2:
            emb = emb[None]
    unc = None
    if a.uncond is not None:
        unc = torch.load(a.uncond, map_location="cpu", weights_only=True)
        unc = unc[None] if unc.dim() == 2 else unc
    if a.keypoints is not None and a.pose_from is not None:
        ap.error("--keypoints and --pose-from are mutually exclusive")
    if (a.keypoints is None and a.pose_from is None) != (a.keypoint_indices is None):
        ap.error("--keypoints or --pose-from go together with --keypoint-indices")
    if a.pose_from is not None and not os.path.isfile(a.pose_from):
        ap.error(f"--pose-from: no such image: {a.pose_from!r}")
    kp = {}
    if a.keypoint_indices is not None:
        def listed(text, number, what):
            if os.path.exists(text):
                return torch.load(text, map_location="cpu", weights_only=True)
            try:
                return torch.tensor([[number(v) for v in part.split(",")] for part in text.split(";")])
            except ValueError:
                ap.error(f"{what}: neither a file nor numbers: {text!r}")
        window = [float(v) for v in a.keypoint_steps.split(",")]
        if len(window) != 2:
            ap.error("--keypoint-steps takes lo,hi")
        kp = dict(keypoint_indices=listed(a.keypoint_indices, int, "--keypoint-indices").reshape(-1).long(),
                  keypoint_scale=a.keypoint_scale, keypoint_steps=tuple(window))
        if a.keypoints is not None:
            kp.update(keypoints=listed(a.keypoints, float, "--keypoints").float(), keypoint_sigma=a.keypoint_sigma)
    if a.batch < 1:
        ap.error("--batch must be at least 1")
    if not 0.0 <= a.eta <= 1.0:
        ap.error("--eta must be in [0, 1]")
    if a.eta > 0:
        if a.sampler not in (None, "ddim"):
            ap.error("--eta belongs to --sampler ddim")
        a.sampler = "ddim"
    ldm, controllers, _ = load_ldm(a.device, a.model, decoder=True, prediction_type=a.prediction_type,
                                   text_encoder=a.prompt is not None or a.negative_prompt is not None)
    if emb is None:
        emb = ptp_utils.encode_prompt(ldm, [a.prompt])
        emb = emb[0] if isinstance(emb, tuple) else emb
    controller = next(iter(controllers.values()))
    if a.pose_from is not None:
        from stablekeypoints_amd.custom_images import CustomDataset
        example = CustomDataset.load_image(a.pose_from, a.size)
        shape = (1, ptp_utils._in_channels(ldm.unet), a.size // 8, a.size // 8)
        noise = torch.randn(shape, generator=torch.Generator().manual_seed(a.seed)).to(ldm.device)
        kp.update(target_maps=ptp_utils.pose_targets(ldm, example, emb, kp["keypoint_indices"], noise_level=a.pose_noise_level, noise=noise),
                  target_energy=a.pose_energy)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for first in range(0, a.n, a.batch):
        ids = range(first, min(first + a.batch, a.n))
        gens = [torch.Generator().manual_seed(a.seed + i) for i in ids]
        trace = []
        image, _ = ptp_utils.text2image_ldm_stable(ldm, emb, controller, num_inference_steps=a.steps, guidance_scale=a.guidance,
                                                   generator=gens[0] if a.batch == 1 else gens, height=a.size, width=a.size,
                                                   uncond_embedding=unc, uncond_prompt=a.negative_prompt, sampler=a.sampler, eta=a.eta,
                                                   keypoint_trace=trace, capture=a.capture, **kp)
        for row, i in enumerate(ids):
            if trace:
                print(f"image {i}: keypoint energy {float(trace[0][row]):.6f} at the first guided step, {float(trace[-1][row]):.6f} "
                      f"at the last of {len(trace)}")
            path = f"{a.out}_{i}" + (".png" if Image is not None else ".npy")
            if Image is not None:
                Image.fromarray(image[row]).save(path)
            else:
                np.save(path, image[row])
            print(path)


if __name__ == "__main__":
    main()
