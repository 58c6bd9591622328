"""The reference's eval.py: arg-max helpers with its names / semantics (eval.py:39-111) on the HIP token-statistics kernel
(csrc/skp_select_loss.hip), the augmented inference (:197-355), and the evaluation stage -- `locate_keypoints` (one fused pass from a
whole group's maps to locations, csrc/skp_locate.hip), `find_corresponding_points` (:159-195), `swap_points` (:360-371),
`keypoint_errors` (the five dataset metrics of :452-494) and `evaluate` (:374-523).  NOT built: the reference's dataset classes
(`evaluate` takes any `{"img", "kpts"[, "visibility"]}` dataset, e.g. `custom_images.AnnotatedImages`), wandb logging, and the debug
figure of `visualize=True`."""
from __future__ import annotations

import torch

from . import ops
from . import routes as _routes


def _points(flat: torch.Tensor, w: int) -> torch.Tensor:
    return torch.stack([flat // w, flat % w], dim=-1).to(torch.float32) + 0.5


def find_max_pixel(map):
    """[B,h,w] -> [B,2] = (row+0.5, col+0.5) of the first maximal element (eval.py:39-60)."""
    am, _ = ops.token_stats(map, num_subjects=1, want_kl=False)
    return _points(am[0].long(), map.shape[-1])


def find_k_max_pixels(map, num=3):
    """[B,h,w] -> [num,B,2]: repeated arg-max with 0.05*h radius masking (eval.py:62-81)."""
    am, _ = ops.token_stats(map, num_subjects=num, want_kl=False)
    return _points(am.long(), map.shape[-1])


def mask_radius(map, max_coords, radius):
    """eval.py:83-111 (elementwise helper, kept for API parity; the fused kernels mask internally)."""
    b, h, w = map.shape
    xs = torch.arange(w, device=map.device).view(1, 1, w)
    ys = torch.arange(h, device=map.device).view(1, h, 1)
    d2 = (xs - max_coords[:, 1].view(b, 1, 1)) ** 2 + (ys - max_coords[:, 0].view(b, 1, 1)) ** 2
    return map * (d2 > radius ** 2).float()


def pixel_from_weighted_avg(heatmaps, distance=5):
    """eval.py:113-155: intensity-weighted mean location within `distance` px of the arg-max (+0.5);
    like the reference this ZEROES the far pixels of `heatmaps` in place."""
    b, m, n = heatmaps.shape
    if distance != -1:
        mx = find_max_pixel(heatmaps)
        x_max, y_max = mx[:, 0].long(), mx[:, 1].long()
        x = torch.arange(0, m, device=heatmaps.device).float().view(1, m, 1)
        y = torch.arange(0, n, device=heatmaps.device).float().view(1, 1, n)
        dist = torch.sqrt((x - x_max.view(b, 1, 1)) ** 2 + (y - y_max.view(b, 1, 1)) ** 2)
        heatmaps[dist > distance] = 0.0
    total = torch.sum(heatmaps, dim=[1, 2], keepdim=True)
    norm = heatmaps / (total + 1e-6)
    x = torch.arange(0, m, device=heatmaps.device).float().view(1, m, 1)
    y = torch.arange(0, n, device=heatmaps.device).float().view(1, 1, n)
    return torch.stack([torch.sum(x * norm, dim=[1, 2]), torch.sum(y * norm, dim=[1, 2])], dim=-1) + 0.5


def run_image_with_context_augmented(ldm, image, context, indices, device="cuda",
                                     from_where=["down_cross", "mid_cross", "up_cross"], layers=[0, 1, 2, 3, 4, 5],
                                     augmentation_iterations=20, noise_level=-1, augment_degrees=30,
                                     augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), visualize=False,
                                     controllers=None, num_gpus=1, save_folder="outputs", upscale_size=512,
                                     thetas=None, noise=None, shard_over_ranks=False, routes="off"):
    """eval.py:197-355: maps of the selected tokens averaged over random affine views of ONE image.

    Reference loop: per augmentation -> UNet forward -> collect_maps(indices, upsample_res=upscale_size) ->
    inverse-warp the maps and a ones-mask -> accumulate; result = sum/count with NaN -> 0.
    Here all views go through the network as ONE batch (early exit, fused map kernel); gather / resize / unwarp
    stay linear ops applied after the layer/head mean.  The view count is the reference's
    `(augmentation_iterations // num_gpus) * num_gpus`.

    By default every rank that calls this processes ALL views of ITS image (callers shard the images over ranks, as
    `find_best_indices` / `optimize_embedding` do): no collective.  `shard_over_ranks=True` is for the
    opposite layout -- every rank holds the SAME image: rank 0 draws all affine matrices and all noise and broadcasts
    them, rank r takes views r, r+world, ... and the un-warped sum and the coverage count ([K,S,S] each) are
    all-reduced before the division, so the ensemble is the same `n` views as on one GPU and every rank returns the
    same averaged maps; a view count that does not divide by the world size raises.
    `thetas` [n,2,3] / `noise` [n,4,h,w] inject the draws for ALL n views (parity tests).
    `routes`: "off" | "report" | "strict" -- the route ledger's rule for this call (`routes.guard`): "report" resets the ledger
    first, so that `routes.table()` afterwards describes this call; "strict" also raises `routes.UnexpectedRoute` at the gate that
    leaves the HIP kernels for a route outside `routes.DOCUMENTED_LIBRARY_ROUTES`."""
    with _routes.guard(routes):
        return _run_image_with_context_augmented(ldm, image, context, indices, device, from_where, layers, augmentation_iterations, noise_level, augment_degrees, augment_scale,
                                                 augment_translate, visualize, controllers, num_gpus, save_folder, upscale_size, thetas, noise,
                                                 shard_over_ranks)


@torch.no_grad()
def _run_image_with_context_augmented(ldm, image, context, indices, device="cuda",
                                     from_where=["down_cross", "mid_cross", "up_cross"], layers=[0, 1, 2, 3, 4, 5],
                                     augmentation_iterations=20, noise_level=-1, augment_degrees=30,
                                     augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), visualize=False,
                                     controllers=None, num_gpus=1, save_folder="outputs", upscale_size=512,
                                     thetas=None, noise=None, shard_over_ranks=False):
    import numpy as np
    from . import dist as skp_dist
    from .invertable_transform import RandomAffineWithInverse
    if visualize:
        raise NotImplementedError("plotting is out of scope (SURVEY.md 2.1 row 14)")
    dev, controller = next(iter(controllers.items()))
    if isinstance(image, np.ndarray):
        image = torch.from_numpy(image).permute(2, 0, 1)
    image = image.to(device=dev, dtype=torch.float32)
    n = (augmentation_iterations // num_gpus) * num_gpus
    if n < 1:
        raise ValueError(f"augmentation_iterations ({augmentation_iterations}) is smaller than num_gpus ({num_gpus})")
    world = skp_dist.world_size() if shard_over_ranks else 1
    if n % world:
        raise ValueError(f"{n} augmented views do not divide over {world} ranks")
    tr = RandomAffineWithInverse(degrees=augment_degrees, scale=augment_scale, translate=augment_translate)
    if thetas is None:
        thetas = tr.sample_theta(n)                                # host RNG, 4 uniforms per view (invertable_transform.py:42-52)
    thetas = torch.as_tensor(thetas, dtype=torch.float32)
    if noise is None:
        noise = torch.randn(n, 4, image.shape[-2] // 8, image.shape[-1] // 8, device=dev)
    noise = noise.to(dev)
    if world > 1:                                                  # one ensemble for the whole job: rank 0's draws
        thetas, noise = thetas.to(dev).contiguous(), noise.contiguous()
        skp_dist.broadcast_(thetas, 0)
        skp_dist.broadcast_(noise, 0)
        r = skp_dist.rank()
        thetas, noise = thetas[r::world].cpu(), noise[r::world]
    tot, num = _augmented_group(ldm, image[None], context, indices, controller, dev, layers, noise_level, tr, thetas, noise,
                                upscale_size, finish=(world == 1))
    if world == 1:
        return tot[0]
    return finish_augmented(tot[0], num[0][None].expand_as(tot[0]).contiguous(), reduce=True)


def _augmented_group(ldm, images, context, indices, controller, dev, layers, noise_level, tr, thetas, noise, upscale_size,
                     finish=True):
    """`images` [m,3,H,W], `thetas` [m*n,2,3] / `noise` [m*n,4,h,w] (image-major: the n views of image 0, then image 1 ...)
    -> (sum or sum/count [m,K,S,S], count [m,S,S]).  All m*n views are ONE network batch; per image one fused
    resize + un-warp + accumulate launch."""
    from . import ptp_utils
    from ._maps import collect_maps_batched
    from .invertable_transform import RandomAffineWithInverse
    m = images.shape[0]
    n = thetas.shape[0] // m
    views = tr(images.repeat_interleave(n, dim=0), theta=thetas)
    ptp_utils.find_pred_noise(ldm, views, context.to(dev), noise_level=noise_level, device=dev, noise=noise,
                              early_exit=True, controllers={dev: controller})
    idx = torch.as_tensor(indices, device=dev).long()
    maps = collect_maps_batched(controller, layers=layers, indices=idx)    # [m*n,K,R,R]: only the selected tokens' maps
    # resize R -> upscale_size, un-warp the maps and a ones mask, sum over the views: ONE kernel (the reference's four
    # [n,K,S,S] intermediates are never materialised); a single rank gets sum / count straight from it
    theta_inv = RandomAffineWithInverse.invert(thetas.to(torch.float32))
    tots, nums = [], []
    for i in range(m):
        tot, num = ops.unwarp_accumulate(maps[i * n:(i + 1) * n], theta_inv[i * n:(i + 1) * n], int(upscale_size), finish=finish)
        tots.append(tot)
        nums.append(num)
    return torch.stack(tots), torch.stack(nums)


@torch.no_grad()
def run_images_with_context_augmented(ldm, images, context, indices, controllers=None, layers=[0, 1, 2, 3, 4, 5],
                                      augmentation_iterations=20, noise_level=-1, augment_degrees=30,
                                      augment_scale=(0.9, 1.1), augment_translate=(0.1, 0.1), num_gpus=1, upscale_size=512,
                                      thetas=None, noise=None):
    """`run_image_with_context_augmented` for SEVERAL images in one network batch (the dataset loops of
    keypoint_regressor.py:160-196 / eval.py:424-446 call it once per image): images [m,3,H,W] -> [m,K,S,S].  Per image the
    result is what the single-image function returns for the same draws (`thetas` [m*n,2,3], `noise` [m*n,4,h,w],
    image-major)."""
    from .invertable_transform import RandomAffineWithInverse
    dev, controller = next(iter(controllers.items()))
    images = images.to(device=dev, dtype=torch.float32)
    m = images.shape[0]
    n = (augmentation_iterations // num_gpus) * num_gpus
    if n < 1:
        raise ValueError(f"augmentation_iterations ({augmentation_iterations}) is smaller than num_gpus ({num_gpus})")
    tr = RandomAffineWithInverse(degrees=augment_degrees, scale=augment_scale, translate=augment_translate)
    if thetas is None:
        thetas = tr.sample_theta(m * n)
    thetas = torch.as_tensor(thetas, dtype=torch.float32)
    if noise is None:
        noise = torch.randn(m * n, 4, images.shape[-2] // 8, images.shape[-1] // 8, device=dev)
    tot, _ = _augmented_group(ldm, images, context, indices, controller, dev, layers, noise_level, tr, thetas, noise.to(dev),
                              upscale_size, finish=True)
    return tot


def finish_augmented(tot, num, reduce=True):
    """eval.py:343-353; with `reduce` across ranks: SUM all-reduce of the un-warped map sum and of the coverage count
    (one exchange of 2 x [K,S,S] floats), then sum / count with 0/0 -> 0."""
    from . import dist as skp_dist
    if reduce and skp_dist.world_size() > 1:
        both = torch.stack([tot, num])
        skp_dist.allreduce_sum_(both)
        tot, num = both[0], both[1]
    out = tot / num
    out[out != out] = 0
    return out


# ---------------------------------------------------------------------------------------------
# evaluation stage: maps -> locations -> regressed keypoints -> dataset error       eval.py:113-195, 360-523
# ---------------------------------------------------------------------------------------------
STRATEGIES = ("argmax", "weighted_avg")
METHODS = ("inter_eye_distance", "visible", "mean_average_error", "pck", "orientation_invariant")


def locate_formula(maps, strategy="argmax", distance=5):
    """The definition of include/skp_locate.h in torch ops, in the dtype of `maps` and without writing into it: [N,h,w] ->
    (loc [N,2] = (row, col) in pixels, flat int64 [N]).  The op order is the reference's (eval.py:113-155: normalise by the
    window's sum + 1e-6, then the weighted sums); the window test is the reference's expression in fp32, whatever the dtype of the
    maps.  In fp64 this is the definition."""
    n, h, w = maps.shape
    flat = torch.argmax(maps.reshape(n, -1), dim=-1)
    rs, cs = flat // w, flat % w
    if strategy == "argmax":
        return torch.stack([rs, cs], dim=-1).to(maps.dtype) + 0.5, flat
    r = torch.arange(h, device=maps.device).view(1, h, 1)
    c = torch.arange(w, device=maps.device).view(1, 1, w)
    m = maps
    if distance != -1:
        d2 = (r - rs.view(n, 1, 1)) ** 2 + (c - cs.view(n, 1, 1)) ** 2
        inside = torch.sqrt(d2.to(torch.float32)) <= torch.tensor(float(distance), dtype=torch.float32, device=maps.device)
        m = torch.where(inside, maps, torch.zeros((), dtype=maps.dtype, device=maps.device))
    norm = m / (torch.sum(m, dim=[1, 2], keepdim=True) + 1e-6)
    r, c = r.to(maps.dtype), c.to(maps.dtype)
    return torch.stack([torch.sum(r * norm, dim=[1, 2]), torch.sum(c * norm, dim=[1, 2])], dim=-1) + 0.5, flat


def locate_keypoints(maps, strategy="argmax", distance=5):
    """[..., h, w] -> [..., 2]: per map (row + 0.5, col + 0.5) of the first maximal element (`argmax`: eval.py:39-60), or the
    intensity-weighted mean location over the pixels within `distance` of it, -1 for the whole map (`weighted_avg`:
    eval.py:113-155), in pixels.  One launch for all the maps (ops.locate, include/skp_locate.h); `maps` is not modified, unlike
    `pixel_from_weighted_avg`'s argument.  Host tensors and other dtypes evaluate `locate_formula`."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {STRATEGIES}, got {strategy!r}")
    if maps.dim() < 2 or maps.numel() == 0:
        raise ValueError(f"locate_keypoints: expected [..., h, w] with elements, got {tuple(maps.shape)}")
    if strategy == "weighted_avg" and not (distance >= 0 or distance == -1):
        raise ValueError(f"distance must be >= 0, or -1 for the whole map, got {distance!r}")
    lead, (h, w) = maps.shape[:-2], maps.shape[-2:]
    if maps.is_cuda and maps.dtype == torch.float32:
        _routes.note("eval.locate", "locate")
        loc, _ = ops.locate(maps, STRATEGIES.index(strategy), distance)
    else:
        _routes.note("eval.locate", "host")
        loc, _ = locate_formula(maps.detach().reshape(-1, h, w), strategy, distance)
    return loc.reshape(*lead, 2)


def find_corresponding_points(maps, num_points=10):
    """eval.py:159-195: maps [n,T,h,w] -> (points [n,num_points,2] = (row, col) in [0, 1], the `num_points` tokens of lowest entropy).
    The entropy is that of torch.distributions.Categorical(probs = softmax over the pixels) per map (probabilities renormalised,
    their logarithm clamped at the dtype's eps), summed over the images; the points are the arg-max locations of the chosen
    tokens' maps, one locator launch, divided by (h, w): what `visualize.plot_point_correspondences` takes (the reference returns
    them in pixels)."""
    n, T, h, w = maps.shape
    sm = torch.softmax(maps.reshape(n * T, h * w), dim=-1)
    probs = sm / sm.sum(dim=-1, keepdim=True)
    eps = torch.finfo(probs.dtype).eps
    entropy = -(torch.log(probs.clamp(min=eps, max=1 - eps)) * probs).sum(dim=-1).reshape(n, T).sum(dim=0)
    chosen = torch.argsort(entropy)[:num_points]
    pts = locate_keypoints(maps[:, chosen].contiguous(), "argmax")
    return pts / torch.tensor([float(h), float(w)], dtype=pts.dtype, device=pts.device), chosen


SWAP_PAIRS = [(1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (17, 25), (18, 26), (19, 27), (20, 28), (21, 28), (22, 30), (23, 31)]


def swap_points(points):
    """eval.py:360-371: the left / right swap of the 32 Human3.6M joints, points [B,N,D].  The pairs are the reference's as
    written, (21, 28) after (20, 28) included: joint 28 ends up taking 21, 20 takes 28 and 21 takes 28."""
    permutation = list(range(points.shape[1]))
    for a, b in SWAP_PAIRS:
        permutation[a] = b
        permutation[b] = a
    return points[:, permutation, :]


def keypoint_errors(locations, regressor, gt, visibility=None, method="inter_eye_distance"):
    """eval.py:452-494 for all images at once: locations [N,K,2] in [0, 1], regressor [2K,2G], gt [N,G,2] in [0, 1], visibility
    [N,G] or None (ones) -> the error of every image [N], in torch on the device and in the dtype of `locations`.
        est = ((locations.view(N, -1) - 0.5) @ regressor + 0.5).view(N, G, 2);  l2 = |est - gt| per keypoint
        inter_eye_distance      mean of l2 / |gt[0] - gt[1]|
        visible                 sum(l2 vis) / sum(vis)                (an image without a visible keypoint: NaN, as the reference)
        mean_average_error      sum(l2 vis), est and gt times 256
        pck                     mean of (l2 < 6), est and gt times 256
        orientation_invariant   128 min(mean l2, mean l2 of `swap_points(est)`)
    Another method raises ValueError (the reference dies with a NameError after its first image)."""
    if method not in METHODS:
        raise ValueError(f"evaluation method must be one of {METHODS}, got {method!r}")
    N = locations.shape[0]
    regressor, gt = regressor.to(locations), gt.to(locations)
    est = ((locations.reshape(N, -1) - 0.5) @ regressor + 0.5).reshape(N, -1, 2)
    if est.shape != gt.shape:
        raise ValueError(f"the regressor gives {tuple(est.shape)} keypoints, the annotations are {tuple(gt.shape)}")
    if method in ("mean_average_error", "pck"):
        est, gt = est * 256, gt * 256
    l2 = (est - gt).norm(dim=-1)
    if method == "inter_eye_distance":
        return (l2 / torch.sqrt(torch.sum((gt[:, 0] - gt[:, 1]) ** 2, dim=-1, keepdim=True))).mean(dim=1)
    if method in ("visible", "mean_average_error"):
        vis = torch.ones_like(l2) if visibility is None else visibility.to(l2)
        total = (l2 * vis).sum(dim=1)
        return total / vis.sum(dim=1) if method == "visible" else total
    if method == "pck":
        return (l2 < 6).to(l2.dtype).mean(dim=1)
    mean, swapped = l2.mean(dim=1), (swap_points(est) - gt).norm(dim=-1).mean(dim=1)
    return torch.where(swapped < mean, swapped, mean) * 128


@torch.no_grad()
def evaluate(ldm, context, indices, regressor, args, controllers, num_gpus, from_where=["down_cross", "mid_cross", "up_cross"],
             dataset=None, routes="off", draws=None):
    """eval.py:374-523 -> (mean error, all_errors [N] on the host).  Per image of the test set: the augmented maps of the voted
    tokens, their locations (`args.max_loc_strategy`), the regressed keypoints, the error under `args.evaluation_method`
    (`keypoint_errors`).  The dataset loop is `precompute_all_keypoints`'s with `batched_locator=True`: groups of
    `args.images_per_forward` images in one network batch and one locator launch, the images sharded over the ranks, one gather;
    every image of the dataset is taken (`args.max_num_points` bounds the regressor's training set, not this).
    `all_errors.pt` goes to `args.save_folder` when that is set (rank 0 writes).
    ORDER: the errors come out in DATASET order (all_errors[i] belongs to dataset[i]); the reference's come out in the order of its
    shuffled loader, which it does not record.  The mean is the same.
    `dataset`: any `{"img", "kpts"[, "visibility"]}` dataset (default: `build_dataset(args)`; one without "kpts" raises).
    `draws = (order, noise, thetas)`: as `precompute_all_keypoints` (parity tests; the errors then come out in `order`).
    `routes`: "off" | "report" | "strict", the route ledger's rule for this call (`routes.guard`)."""
    import os
    from . import dist as skp_dist
    from . import keypoint_regressor as KR
    method = getattr(args, "evaluation_method", "inter_eye_distance")
    if method not in METHODS:
        raise ValueError(f"evaluation method must be one of {METHODS}, got {method!r}")
    with _routes.guard(routes):
        source, targets, vis = KR._precompute_all_keypoints(ldm, context, indices, args, controllers, num_gpus, from_where, dataset,
                                                            draws, batched_locator=True, whole_dataset=True)
        if targets is None:
            raise ValueError("evaluate: the dataset's items carry no 'kpts'")
        errors = keypoint_errors(source, regressor.to(source.device), targets.to(source.device), vis, method).cpu()
    folder = getattr(args, "save_folder", None)
    if folder and skp_dist.rank() == 0:
        os.makedirs(folder, exist_ok=True)
        torch.save(errors, os.path.join(folder, "all_errors.pt"))
    return float(errors.mean()), errors
