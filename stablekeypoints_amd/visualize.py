"""Keypoint visualisation with the reference's names (visualize.py:40-248): numbered markers on a grid of images, one heat-map grid
per keypoint, optional grids of regressed and annotated keypoints -- as PNG files, drawn by one fused HIP pass instead of matplotlib.

From (images, maps, points) to pixels is `ops.map_range` + `ops.overlay_u8` (csrc/skp_overlay.hip): clamp -> min-max normalised map
through a colour table, blended at `alpha` -> anti-aliased discs with a white ring and the keypoint's number from a 5 x 7 font ->
uint8 NHWC straight into the canvas of a grid.  The maps [n,K,512,512] never leave the device; what crosses to the host is the
finished canvas.  `overlay_formula` is the same four steps in torch in the dtype of its inputs: the host route (CPU tensors), and
the written-out definition the kernel is tested against (include/skp_overlay.h states it per pixel).

`VIRIDIS`, `COLORS` and `FONT_5X7` are this project's own tables (the reference takes its colours and digits from matplotlib): nine
nodes approximating the viridis colour map, a ten-colour cycle, and the digits 0-9 as seven 5-bit rows each.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import torch

from . import routes as _routes

VIRIDIS = torch.tensor([[0.267, 0.004, 0.329], [0.278, 0.176, 0.482], [0.231, 0.322, 0.545], [0.173, 0.447, 0.557],
                        [0.129, 0.569, 0.549], [0.157, 0.682, 0.502], [0.369, 0.788, 0.384], [0.678, 0.863, 0.188],
                        [0.992, 0.906, 0.145]], dtype=torch.float32)
COLORS = torch.tensor([[0.90, 0.10, 0.12], [0.12, 0.45, 0.85], [0.15, 0.65, 0.22], [0.95, 0.55, 0.05], [0.55, 0.25, 0.75],
                       [0.05, 0.70, 0.75], [0.90, 0.30, 0.65], [0.70, 0.70, 0.10], [0.55, 0.35, 0.22], [0.42, 0.42, 0.47]],
                      dtype=torch.float32)
_FONT_ROWS = ("01110 10001 10011 10101 11001 10001 01110",      # 0
              "00100 01100 00100 00100 00100 00100 01110",      # 1
              "01110 10001 00001 00010 00100 01000 11111",      # 2
              "11110 00001 00001 01110 00001 00001 11110",      # 3
              "00010 00110 01010 10010 11111 00010 00010",      # 4
              "11111 10000 11110 00001 00001 10001 01110",      # 5
              "00110 01000 10000 11110 10001 10001 01110",      # 6
              "11111 00001 00010 00100 01000 01000 01000",      # 7
              "01110 10001 10001 01110 10001 10001 01110",      # 8
              "01110 10001 10001 01111 00001 00010 01100")      # 9
FONT_5X7 = torch.tensor([[int(r, 2) for r in g.split()] for g in _FONT_ROWS], dtype=torch.uint8)      # [10,7], leftmost column = bit 4
MAX_POINTS = 100                                                 # two-digit labels


def _f32(v) -> float:
    """A Python number as the float the C entry receives."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def marker_size(H: int, radius=None, ring=None):
    """(radius, ring) in pixels: 9 and 1.5 at 512 rows, scaled with the image, at least 3 and 1; rounded to float32."""
    radius = max(3.0, 9.0 * H / 512.0) if radius is None else radius
    ring = max(1.0, 1.5 * H / 512.0) if ring is None else ring
    return _f32(radius), _f32(ring)


def glyph_scale(radius: float, digits: int) -> int:
    """Largest integer scale, at least 1, at which a label of `digits` digits (5 or 5 + 1 + 5 columns, 7 rows) fits inside the disc."""
    bw = 5 if digits == 1 else 11
    return max(1, int(radius / (0.5 * (bw * bw + 49) ** 0.5)))


def cycle_colors(K: int, colors=COLORS):
    colors = torch.as_tensor(colors, dtype=torch.float32)
    return colors[torch.arange(K) % colors.shape[0]]


def range_formula(maps):
    """[B,S,S] -> [B,2] = (min, max) ignoring NaN, (0, 0) for a map of only NaN: `ops.map_range` in torch."""
    flat = maps.reshape(maps.shape[0], -1)
    nan = torch.isnan(flat)
    lo = torch.where(nan, torch.full_like(flat, float("inf")), flat).amin(dim=1)
    hi = torch.where(nan, torch.full_like(flat, float("-inf")), flat).amax(dim=1)
    empty = nan.all(dim=1)
    return torch.stack([torch.where(empty, torch.zeros_like(lo), lo), torch.where(empty, torch.zeros_like(hi), hi)], dim=1)


def _taps(n_dst, n_src, dt):
    """Source rows of F.interpolate(mode="bilinear", align_corners=False): (index 0, index 1, weight of index 1)."""
    ratio = torch.tensor(n_src, dtype=dt) / torch.tensor(n_dst, dtype=dt)
    src = (ratio * (torch.arange(n_dst, dtype=dt) + 0.5) - 0.5).clamp(min=0)
    i0 = src.long().clamp(max=n_src - 1)
    return i0, (i0 + 1).clamp(max=n_src - 1), src - i0.to(dt)


def overlay_formula(img, maps=None, points=None, *, alpha=0.7, cmap=VIRIDIS, colors=None, glyphs=FONT_5X7, radius=None, ring=None,
                    labels=True, rng=None):
    """The four steps of include/skp_overlay.h in torch, in the dtype of `img`: img [B,3,H,W], maps [B,S,S] or None, points [B,K,2]
    (row, col) in image fractions or None -> uint8 [B,H,W,3].  What the kernel computes in fp32, operation by operation (the kernel is
    built without fma contraction, as torch rounds every op); in fp64 it is the definition."""
    dt = img.dtype
    B, _, H, W = img.shape
    radius, ring = marker_size(H, radius, ring)
    c = img.clamp(0, 1).permute(0, 2, 3, 1).clone()                                   # [B,H,W,3]
    if maps is not None:
        maps = maps.to(dt)
        S = maps.shape[-1]
        lut = torch.as_tensor(cmap).to(dt)
        rng = range_formula(maps) if rng is None else rng.to(dt)
        if S == H and S == W:
            m = maps
        else:
            r0, r1, ty = _taps(H, S, dt)
            c0, c1, tx = _taps(W, S, dt)
            top = (1 - tx) * maps[:, r0][:, :, c0] + tx * maps[:, r0][:, :, c1]
            bot = (1 - tx) * maps[:, r1][:, :, c0] + tx * maps[:, r1][:, :, c1]
            m = (1 - ty).view(1, H, 1) * top + ty.view(1, H, 1) * bot
        lo, hi = rng[:, 0].view(B, 1, 1), rng[:, 1].view(B, 1, 1)
        n = ((m - lo) / (hi - lo)).clamp(0, 1)
        n = torch.where((hi > lo) & ~torch.isnan(m) & ~torch.isnan(n), n, torch.zeros_like(n))
        L = lut.shape[0]
        t = n * (L - 1)
        i = t.long().clamp(max=L - 2)
        colour = lut[i] + (t - i.to(dt)).unsqueeze(-1) * (lut[i + 1] - lut[i])
        a = torch.tensor(_f32(alpha), dtype=dt)
        c = (1 - a) * c + a * colour
    if points is not None and points.shape[1] > 0:
        points = points.to(dt)
        K = points.shape[1]
        if K > MAX_POINTS:
            raise ValueError(f"at most {MAX_POINTS} points per image (two-digit labels), got {K}")
        cols = (cycle_colors(K) if colors is None else torch.as_tensor(colors)).to(dt)
        glyphs = torch.as_tensor(glyphs).long()
        r_ring, r_disc = torch.tensor(radius + ring + 0.5).to(dt), torch.tensor(radius + 0.5).to(dt)
        yc, xc = (torch.arange(H, dtype=dt) + 0.5).view(1, H, 1), (torch.arange(W, dtype=dt) + 0.5).view(1, 1, W)
        yi, xi = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
        for j in range(K):
            py, px = points[:, j, 0] * H, points[:, j, 1] * W
            valid = ~(torch.isnan(py) | torch.isnan(px))
            py, px = torch.where(valid, py, torch.zeros_like(py)), torch.where(valid, px, torch.zeros_like(px))
            dy, dx = yc - py.view(B, 1, 1), xc - px.view(B, 1, 1)
            d = torch.sqrt(dy * dy + dx * dx)
            v = valid.view(B, 1, 1).to(dt)
            ar, ad = ((r_ring - d).clamp(0, 1) * v).unsqueeze(-1), ((r_disc - d).clamp(0, 1) * v).unsqueeze(-1)
            c = c + ar * (1 - c)
            c = c + ad * (cols[j] - c)
            if labels:
                fs, bw = glyph_scale(radius, 1 if j < 10 else 2), (5 if j < 10 else 11)
                oy = torch.floor(py - 3.5 * fs + 0.5).long().view(B, 1, 1)
                ox = torch.floor(px - 0.5 * (bw * fs) + 0.5).long().view(B, 1, 1)
                gy, gx = yi - oy, xi - ox
                inside = (gy >= 0) & (gy < 7 * fs) & (gx >= 0) & (gx < bw * fs) & valid.view(B, 1, 1)
                gy, gx = gy.clamp(0, 7 * fs - 1) // fs, gx.clamp(0, bw * fs - 1) // fs
                if bw == 5:
                    bit = (glyphs[j][gy] >> (4 - gx)) & 1
                else:
                    tens = (glyphs[j // 10][gy] >> (4 - gx.clamp(max=4))) & 1
                    ones = (glyphs[j % 10][gy] >> (4 - (gx - 6).clamp(min=0))) & 1
                    bit = torch.where(gx < 5, tens, torch.where(gx > 5, ones, torch.zeros_like(ones)))
                on = (inside & (bit == 1)).expand(B, H, W).unsqueeze(-1)
                c = torch.where(on, c + ad * (1 - c), c)
    return ((c * 255).to(torch.int32) & 255).to(torch.uint8)


_consts = {}


def _on_device(name, t, dev):
    """The module's own tables on `dev`, uploaded once."""
    key = (name, str(dev))
    if key not in _consts:
        _consts[key] = t.to(dev).contiguous()
    return _consts[key]


def overlay(img, maps=None, points=None, *, alpha=0.7, cmap=VIRIDIS, colors=None, radius=None, ring=None, labels=True, out=None,
            origin=(0, 0), cols=1, gap=0):
    """img [B,3,H,W] (or [3,H,W]) in [0, 1], maps [B,S,S] or None, points [B,K,2] (row, col) in [0, 1] or None -> uint8 pixels.
    `out` None: [B,H,W,3].  Otherwise `out` is a uint8 canvas [h, w, 3] (pre-filled by the caller, on the device of `img`) and image
    b is written at origin + (b // cols, b % cols) * (H + gap, W + gap); nothing else of the canvas is touched.
    Device tensors go to the HIP kernels (`ops.map_range`, `ops.overlay_u8`), host tensors to `overlay_formula`; the ledger sites
    `visualize.range` / `visualize.overlay` record which.  Default marker size: `marker_size(H)`."""
    if img.dim() == 3:
        img = img[None]
    B, _, H, W = img.shape
    radius, ring = marker_size(H, radius, ring)
    K = 0 if points is None else points.shape[1]
    if K > MAX_POINTS:
        raise ValueError(f"at most {MAX_POINTS} points per image (two-digit labels), got {K}")
    if img.is_cuda:
        from . import ops
        dev = img.device
        rng = lut = pts = col = None
        if maps is not None:
            maps = maps.to(dev, torch.float32)
            rng = ops.map_range(maps)
            _routes.note("visualize.range", "map_range")
            lut = _on_device("viridis", VIRIDIS, dev) if cmap is VIRIDIS else torch.as_tensor(cmap, dtype=torch.float32).to(dev)
        if K:
            pts = points.to(dev, torch.float32)
            col = cycle_colors(K).to(dev) if colors is None else torch.as_tensor(colors, dtype=torch.float32).to(dev)
        res = ops.overlay_u8(img, maps, rng, lut, alpha, pts, col, _on_device("font", FONT_5X7, dev), radius, ring, labels, out=out,
                             origin=origin, cols=cols, gap=gap)
        _routes.note("visualize.overlay", "overlay_u8")
        return res
    if maps is not None:
        _routes.note("visualize.range", "host")
    _routes.note("visualize.overlay", "host")
    tiles = overlay_formula(img, maps, points, alpha=alpha, cmap=cmap, colors=colors, radius=radius, ring=ring, labels=labels)
    if out is None:
        return tiles
    for b in range(B):
        y, x = origin[0] + (b // cols) * (H + gap), origin[1] + (b % cols) * (W + gap)
        if y + H > out.shape[0] or x + W > out.shape[1]:
            raise ValueError(f"tile {b} at ({y}, {x}) leaves the {tuple(out.shape)} canvas")
        out[y:y + H, x:x + W] = tiles[b]
    return out


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------
def write_png(path, pixels, level: int = 3):
    """uint8 [H,W,3] (tensor or array) -> an 8-bit RGB PNG, filter type 0 on every row; nothing but zlib and struct."""
    a = pixels.detach().cpu().numpy() if torch.is_tensor(pixels) else np.asarray(pixels)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"write_png: expected uint8 [H,W,3], got {a.dtype} {a.shape}")
    h, w, _ = a.shape
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                                     # a filter byte (0) in front of every row
    rows[:, 1:] = a.reshape(h, 3 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + chunk(b"IEND", b""))
    return path


def _stack(imgs):
    return imgs if torch.is_tensor(imgs) else torch.stack([torch.as_tensor(i) for i in imgs])


def _canvas(rows, cols, H, W, gap, device):
    return torch.full((rows * (H + gap) - gap, cols * (W + gap) - gap, 3), 255, dtype=torch.uint8, device=device)


GAP = 4            # white pixels between tiles; a multiple of 4 keeps the four-pixels-per-lane form of the kernel


def save_grid(maps, imgs, name, gap=GAP, alpha=0.7):
    """visualize.py:40-73: a 2 x n canvas, the images on top and the same images under their min-max normalised heat map (alpha 0.7)
    below, white gaps; maps [n,S,S], imgs n x [3,H,W].  Two overlay launches into one canvas.  Returns the canvas (on the host)."""
    imgs = _stack(imgs)
    maps = torch.as_tensor(maps).to(imgs.device)
    n, _, H, W = imgs.shape
    canvas = _canvas(2, n, H, W, gap, imgs.device)
    overlay(imgs, out=canvas, cols=n, gap=gap)
    overlay(imgs, maps, alpha=alpha, out=canvas, origin=(H + gap, 0), cols=n, gap=gap)
    canvas = canvas.cpu()
    write_png(name, canvas)
    return canvas


def plot_point_single(img, points, name):
    """visualize.py:76-103: one image with the numbered points of every person; points [people, K, 2].  The people are drawn one
    after the other, each over the bytes of the one before."""
    img = torch.as_tensor(img)
    points = torch.as_tensor(points)
    out = None
    for p in range(points.shape[0]):
        src = img[None] if out is None else (out.permute(0, 3, 1, 2).to(torch.float32) + 0.5) / 255.0
        out = overlay(src, points=points[p:p + 1].to(img.device))
    out = (overlay(img[None]) if out is None else out)[0].cpu()
    write_png(name, out)
    return out


def plot_point_correspondences(imgs, points, name, height=11, width=9, gap=GAP):
    """visualize.py:105-138: a height x width grid of images with their numbered points, one launch; a tile without an image stays
    white.  points [n,K,2]."""
    imgs = _stack(imgs)[:height * width]
    points = torch.as_tensor(points)[:height * width].to(imgs.device)
    _, _, H, W = imgs.shape
    canvas = _canvas(height, width, H, W, gap, imgs.device)
    overlay(imgs, points=points, out=canvas, cols=width, gap=gap)
    canvas = canvas.cpu()
    write_png(name, canvas)
    return canvas


def visualize_attn_maps(ldm, context, indices, args, controllers, num_gpus, regressor=None,
                        from_where=["down_cross", "mid_cross", "up_cross"], height=11, width=9, dataset=None, draws=None,
                        routes="off", grid_columns=10):
    """visualize.py:140-248: `height * width` images of a shuffled order (image i is `order[i % len(dataset)]`), their augmented maps
    of the `top_k` voted tokens and the locations on them, drawn into `args.save_folder`:
        unsupervised_keypoints.png   the grid of images with numbered markers
        keypoint_%03d.png            per token: the first `grid_columns` images over themselves under that token's heat map
        estimated_keypoints.png      with a regressor: ((points - 0.5) @ regressor) + 0.5
        gt_keypoints.png             when the dataset's items carry "kpts" ((row, col) in [0, 1])
    (PNG where the reference writes PDF.)  The maps come from `run_images_with_context_augmented` in groups of
    `args.images_per_forward` and stay on the device; the locations from `keypoints_from_maps` (`args.max_loc_strategy`; the
    weighted average works on a copy, so the heat maps are drawn from the maps as they came).  `draws = (order, noise [n*a,4,h,w],
    thetas [n*a,2,3])` injects the randomness, as in `precompute_all_keypoints`; `routes` as there.
    Returns (points [n,K,2] on the host, the list of files written)."""
    with _routes.guard(routes):
        return _visualize_attn_maps(ldm, context, indices, args, controllers, num_gpus, regressor, height, width, dataset, draws,
                                    grid_columns)


@torch.no_grad()
def _visualize_attn_maps(ldm, context, indices, args, controllers, num_gpus, regressor, height, width, dataset, draws, grid_columns):
    from .eval import run_images_with_context_augmented
    from .keypoint_regressor import keypoints_from_maps
    from .optimize import build_dataset
    dev, controller = next(iter(controllers.items()))
    if dataset is None:
        dataset = build_dataset(args)
    n = height * width
    n_aug = (args.augmentation_iterations // num_gpus) * num_gpus
    strategy = getattr(args, "max_loc_strategy", "argmax")
    if draws is not None:
        order = [int(i) for i in draws[0]]
        noise, thetas = torch.as_tensor(draws[1]), torch.as_tensor(draws[2], dtype=torch.float32)
    else:
        gen = torch.Generator().manual_seed(getattr(args, "seed", 0) + 1357)
        order, noise, thetas = torch.randperm(len(dataset), generator=gen).tolist(), None, None
    group = max(1, int(getattr(args, "images_per_forward", 4)))
    idx = torch.as_tensor(indices).long()
    imgs, maps, points, gt = [], [], [], []
    for g0 in range(0, n, group):
        pos = list(range(g0, min(n, g0 + group)))
        items = [dataset[order[p % len(order)] % len(dataset)] for p in pos]
        batch = torch.stack([torch.as_tensor(it["img"]) for it in items]).to(dev, torch.float32)
        gt += [torch.as_tensor(it["kpts"]).float().cpu() for it in items if "kpts" in it]
        rows = [r for p in pos for r in range(p * n_aug, (p + 1) * n_aug)]
        m = run_images_with_context_augmented(
            ldm, batch, context, idx, controllers={dev: controller}, layers=args.layers,
            augmentation_iterations=args.augmentation_iterations, noise_level=args.noise_level,
            augment_degrees=args.augment_degrees, augment_scale=args.augment_scale, augment_translate=args.augment_translate,
            num_gpus=num_gpus, upscale_size=512, thetas=None if thetas is None else thetas[rows],
            noise=None if noise is None else noise[rows])                               # [m,K,512,512]
        for i in range(len(pos)):
            points.append(keypoints_from_maps(m[i] if strategy == "argmax" else m[i].clone(), strategy))
        imgs.append(batch)
        maps.append(m)
    imgs, maps, points = torch.cat(imgs), torch.cat(maps), torch.stack(points)
    os.makedirs(args.save_folder, exist_ok=True)
    files = []

    def out(name):
        files.append(os.path.join(args.save_folder, name))
        return files[-1]

    plot_point_correspondences(imgs, points, out("unsupervised_keypoints.png"), height, width)
    cols = min(n, int(grid_columns))
    for k in range(maps.shape[1]):
        save_grid(maps[:cols, k], imgs[:cols], out(f"keypoint_{k:03d}.png"))
    if regressor is not None:
        reg = torch.as_tensor(regressor).to(points.device, points.dtype)
        est = ((points.reshape(n, -1) - 0.5) @ reg) + 0.5
        plot_point_correspondences(imgs, est.reshape(n, -1, 2), out("estimated_keypoints.png"), height, width)
    if len(gt) == n:
        plot_point_correspondences(imgs, torch.stack(gt), out("gt_keypoints.png"), height, width)
    return points.cpu(), files
