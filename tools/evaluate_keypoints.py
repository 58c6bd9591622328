#!/usr/bin/env python
"""The evaluation stage: from annotated images to the number the method is judged by.
    python tools/evaluate_keypoints.py --model DIR|tiny --embedding emb.pt --indices idx.pt --train DIR --test DIR --out DIR
        [--method inter_eye_distance|visible|mean_average_error|pck|orientation_invariant --max-loc-strategy argmax|weighted_avg
         --augmentation-iterations 20 --images-per-forward 4 --max-num-points 50000 --image-size 512 --seed 0]
--train and --test are folders of images with an `annotations.json` (`custom_images.AnnotatedImages`); --embedding and --indices are
what tools/find_keypoints.py writes.  Stages (each reseeds torch's generators from --seed):
  3. `precompute_all_keypoints` over the training folder (one locator launch per group of images)
  4. the regressor of the method (`return_regressor_visible` for visible / mean_average_error, `return_regressor_human36m` for
     orientation_invariant, `return_regressor` otherwise), as float32                          -> regressor.pt
  5. `eval.evaluate` over the test folder                                                       -> all_errors.pt (dataset order)
One JSON line on stdout: {"method", "error", "train_images", "test_images", "keypoints", "files"}.  `main(argv)` returns that dict."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _arguments(argv):
    from stablekeypoints_amd.eval import METHODS, STRATEGIES
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="a checkpoint directory, or a synthetic architecture such as 'tiny'")
    ap.add_argument("--embedding", required=True)
    ap.add_argument("--indices", required=True)
    ap.add_argument("--train", required=True)
    ap.add_argument("--test", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--method", default="inter_eye_distance", choices=METHODS)
    ap.add_argument("--max-loc-strategy", default="argmax", choices=STRATEGIES)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--feature-upsample-res", type=int, default=128)
    ap.add_argument("--augmentation-iterations", type=int, default=20)
    ap.add_argument("--images-per-forward", type=int, default=4)
    ap.add_argument("--max-num-points", type=int, default=50_000)
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def fit_regressor(source, targets, visibility, method):
    """Stage 4 of the reference's main.py (:264-291): source [N,K,2], targets [N,G,2], visibility [N,G] or None -> float32 [2K,2G]."""
    from stablekeypoints_amd import keypoint_regressor as KR
    n = source.shape[0]
    X, Y = source.reshape(n, -1).double().cpu().numpy(), targets.reshape(n, -1).double().cpu().numpy()
    if method in ("visible", "mean_average_error"):
        vis = torch.ones(targets.shape[:2]) if visibility is None else visibility
        W = KR.return_regressor_visible(X, Y, vis.unsqueeze(-1).repeat(1, 1, 2).reshape(n, -1).double().cpu().numpy())
    elif method == "orientation_invariant":
        W = KR.return_regressor_human36m(X, Y)
    else:
        W = KR.return_regressor(X, Y)
    return torch.tensor(W).to(torch.float32)


def main(argv=None):
    a = _arguments(argv)
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd.custom_images import AnnotatedImages
    from stablekeypoints_amd.keypoint_regressor import precompute_all_keypoints
    from stablekeypoints_amd.optimize import default_args
    from stablekeypoints_amd.optimize_token import load_ldm

    os.makedirs(a.out, exist_ok=True)
    train, test = AnnotatedImages(a.train, a.image_size), AnnotatedImages(a.test, a.image_size)
    args = default_args(dataset_name="custom", dataset_loc=a.train, image_size=a.image_size, device=a.device, seed=a.seed,
                        feature_upsample_res=a.feature_upsample_res, augmentation_iterations=a.augmentation_iterations,
                        max_loc_strategy=a.max_loc_strategy, images_per_forward=a.images_per_forward,
                        max_num_points=a.max_num_points, save_folder=a.out, evaluation_method=a.method)
    ldm, controllers, num_gpus = load_ldm(a.device, a.model, feature_upsample_res=a.feature_upsample_res)
    dev = next(iter(controllers))
    embedding = torch.load(a.embedding, map_location="cpu").to(dev)
    indices = torch.load(a.indices, map_location="cpu")

    torch.manual_seed(a.seed + 3)
    source, targets, visibility = precompute_all_keypoints(ldm, embedding, indices, args, controllers, num_gpus, dataset=train,
                                                           batched_locator=True)
    regressor = fit_regressor(source, targets, visibility, a.method)
    files = [os.path.join(a.out, "regressor.pt"), os.path.join(a.out, "all_errors.pt")]
    torch.save(regressor, files[0])

    torch.manual_seed(a.seed + 5)
    mean, errors = E.evaluate(ldm, embedding, indices, regressor.to(dev), args, controllers, num_gpus, dataset=test)
    result = {"method": a.method, "error": mean, "train_images": int(source.shape[0]), "test_images": int(errors.numel()),
              "keypoints": int(targets.shape[1]), "files": files}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
