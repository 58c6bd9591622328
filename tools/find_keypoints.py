#!/usr/bin/env python
"""From a folder of images to keypoints and pictures of them.
    python tools/find_keypoints.py --model DIR|tiny --images DIR --out DIR [--embedding emb.pt] [--indices idx.pt]
        [--num-steps 500 --num-tokens 500 --top-k 10 --augmentation-iterations 20 --max-loc-strategy argmax
         --images-per-forward 4 --grid 11 9 --seed 0]
Stages (each reseeds torch's generators from --seed, so a later stage draws the same numbers whether or not an earlier one ran):
  1. optimise the embedding (`optimize_embedding`) unless --embedding is given            -> embedding.pt
  2. vote the `top_k` tokens (`find_best_indices`) unless --indices is given               -> indices.pt
  3. `precompute_all_keypoints` over the folder
  4. keypoints.json: file name -> K pairs (row, col) in [0, 1], in the file order of `CustomDataset`
  5. keypoints.pt: the same as a tensor [N,K,2]
  6. <stem>_keypoints.png per image (`visualize.plot_point_single`)
  7. the grids of `visualize.visualize_attn_maps`: unsupervised_keypoints.png, keypoint_%03d.png
The run asks the convolution library for its deterministic algorithms (`torch.backends.cudnn.deterministic`, for the length of the run): the few
convolutions that are left to it (routes.DOCUMENTED_LIBRARY_ROUTES: a stride-2 convolution off the kernel's tile) otherwise differ in
the last bit from call to call, which is enough to move an arg-max on a flat map, and a seed would not reproduce keypoints.json.
`main(argv)` returns the list of files written."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


class _Recording(torch.utils.data.Dataset):
    """A dataset that notes which items were read, in order: `precompute_all_keypoints` returns the locations in the order of its
    shuffled pass, and this is that order."""

    def __init__(self, inner):
        self.inner, self.read = inner, []

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, i):
        self.read.append(int(i))
        return self.inner[i]


def main(argv=None):
    a = _arguments(argv)
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return _run(a)
    finally:
        torch.backends.cudnn.deterministic = before


def _arguments(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="a checkpoint directory, or a synthetic architecture such as 'tiny'")
    ap.add_argument("--images", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--embedding")
    ap.add_argument("--indices")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--feature-upsample-res", type=int, default=128)
    ap.add_argument("--num-steps", type=int, default=500)
    ap.add_argument("--num-tokens", type=int, default=500)
    ap.add_argument("--num-indices", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--augmentation-iterations", type=int, default=20)
    ap.add_argument("--max-loc-strategy", default="argmax", choices=["argmax", "weighted_avg"])
    ap.add_argument("--images-per-forward", type=int, default=4)
    ap.add_argument("--grid", type=int, nargs=2, default=[11, 9], metavar=("H", "W"))
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def _run(a):
    from stablekeypoints_amd import visualize
    from stablekeypoints_amd.custom_images import CustomDataset
    from stablekeypoints_amd.keypoint_regressor import find_best_indices, precompute_all_keypoints
    from stablekeypoints_amd.optimize import default_args, optimize_embedding
    from stablekeypoints_amd.optimize_token import load_ldm

    os.makedirs(a.out, exist_ok=True)
    files = []

    def out(name):
        files.append(os.path.join(a.out, name))
        return files[-1]

    dataset = CustomDataset(a.images, image_size=a.image_size)
    args = default_args(dataset_name="custom", dataset_loc=a.images, image_size=a.image_size, device=a.device, seed=a.seed,
                        num_steps=a.num_steps, num_tokens=a.num_tokens, num_indices=a.num_indices, top_k=a.top_k,
                        batch_size=a.batch_size, feature_upsample_res=a.feature_upsample_res,
                        augmentation_iterations=a.augmentation_iterations, max_loc_strategy=a.max_loc_strategy,
                        images_per_forward=a.images_per_forward, max_num_points=len(dataset), save_folder=a.out,
                        furthest_point_num_samples=min(25, a.num_tokens))
    ldm, controllers, num_gpus = load_ldm(a.device, a.model, feature_upsample_res=a.feature_upsample_res)
    dev = next(iter(controllers))

    torch.manual_seed(a.seed + 1)
    if a.embedding:
        embedding = torch.load(a.embedding, map_location="cpu")
    else:
        embedding = optimize_embedding(ldm, args, controllers, num_gpus).cpu()
    torch.save(embedding, out("embedding.pt"))
    embedding = embedding.to(dev)

    torch.manual_seed(a.seed + 2)
    if a.indices:
        indices = torch.load(a.indices, map_location="cpu")
    else:
        indices = find_best_indices(ldm, embedding, args, controllers, num_gpus).cpu()
    torch.save(indices, out("indices.pt"))

    torch.manual_seed(a.seed + 3)
    seen = _Recording(dataset)
    source, _, _ = precompute_all_keypoints(ldm, embedding, indices, args, controllers, num_gpus, dataset=seen)
    source = source.cpu()
    keypoints = torch.empty_like(source)
    keypoints[torch.tensor(seen.read)] = source                  # back to the file order
    names = [os.path.basename(f) for f in dataset.files]
    with open(out("keypoints.json"), "w") as f:
        json.dump({name: keypoints[i].tolist() for i, name in enumerate(names)}, f, indent=1)
    torch.save(keypoints, out("keypoints.pt"))

    for i, name in enumerate(names):
        visualize.plot_point_single(dataset[i]["img"].to(dev), keypoints[i][None], out(os.path.splitext(name)[0] + "_keypoints.png"))

    torch.manual_seed(a.seed + 4)
    _, grids = visualize.visualize_attn_maps(ldm, embedding, indices, args, controllers, num_gpus, height=a.grid[0], width=a.grid[1],
                                             dataset=dataset)
    files += grids
    print(f"{len(names)} images, {keypoints.shape[1]} keypoints each: {len(files)} files under {a.out}")
    return files


if __name__ == "__main__":
    main()
