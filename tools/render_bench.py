#!/usr/bin/env python
"""The overlay renderer (ops.map_range + ops.overlay_u8, csrc/skp_overlay.hip) against the same composition in eager torch, on the
device, in one run:
    python tools/render_bench.py [--images 99] [--maps 10] [--size 512] [--repeats 20] [--json FILE]
  grid    `--images` images x `--maps` heat maps of size^2, as `visualize.save_grid` launches them: per map one range pass over the
          images' maps and one overlay pass into a canvas of tiles
  single  one size^2 image under one map
  points  `--images` images with 10 numbered markers each into a grid canvas (`plot_point_correspondences`; kernel only)
Per pass: microseconds (median of `--repeats` after 3 warm-up rounds, device events around the whole pass), the bytes the pass has to
move (overlay: 12 image + 4 map + 3 out per pixel; range: 4 per pixel), and that rate as a fraction of the copy rate measured in the
same run (a 1 GiB device-to-device copy: the machine's achievable HBM rate).  The working set of the grid case (0.3 GB of images read
once per map, 1 GB of maps) is larger than the last-level cache, the single image is not: its rate is a cache rate, not HBM."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, repeats, warmup=3):
    """Median microseconds of fn() between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return sorted(out)[len(out) // 2]


def eager_range(maps):
    return maps.amin(dim=(1, 2)), maps.amax(dim=(1, 2))


def eager_overlay(img, maps, lo, hi, lut, alpha):
    """The heat-map composition in eager torch: normalised map, colour-mapped map, blend, bytes (NHWC)."""
    L = lut.shape[0]
    n = ((maps - lo.view(-1, 1, 1)) / (hi - lo).view(-1, 1, 1)).clamp(0, 1)
    t = n * (L - 1)
    i = t.long().clamp(max=L - 2)
    colour = lut[i] + (t - i).unsqueeze(-1) * (lut[i + 1] - lut[i])
    c = (1 - alpha) * img.clamp(0, 1).permute(0, 2, 3, 1) + alpha * colour
    return (c * 255).to(torch.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=99)
    ap.add_argument("--maps", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args(argv)
    from stablekeypoints_amd import ops
    from stablekeypoints_amd import visualize as V
    assert torch.cuda.is_available(), "render_bench.py measures on the GPU; there is nothing to measure without one"
    dev = torch.device("cuda", 0)
    n, K, S = a.images, a.maps, a.size
    g = torch.Generator().manual_seed(0)
    imgs = torch.rand(n, 3, S, S, generator=g).to(dev)
    maps = torch.randn(K, n, S, S, generator=g).to(dev)          # map-major: maps[k] is what save_grid gets for token k
    pts = torch.rand(n, 10, 2, generator=g).to(dev)
    lut, colors, font = V.VIRIDIS.to(dev), V.cycle_colors(10).to(dev), V.FONT_5X7.to(dev)
    cols = 11
    rows = (n + cols - 1) // cols
    canvas = torch.full((rows * (S + V.GAP) - V.GAP, cols * (S + V.GAP) - V.GAP, 3), 255, dtype=torch.uint8, device=dev)
    rng = [ops.map_range(maps[k]) for k in range(K)]
    radius, ring = V.marker_size(S)
    pix = n * S * S

    src = torch.empty(1 << 28, device=dev)
    dst = torch.empty_like(src)
    copy_us = timed(lambda: dst.copy_(src), a.repeats)
    copy_rate = 2 * src.numel() * 4 / (copy_us * 1e-6)
    del src, dst

    def k_range():
        for k in range(K):
            ops.map_range(maps[k])

    def k_overlay():
        for k in range(K):
            ops.overlay_u8(imgs, maps[k], rng[k], lut, 0.7, out=canvas, cols=cols, gap=V.GAP)

    def e_range():
        for k in range(K):
            eager_range(maps[k])

    def e_overlay():
        for k in range(K):
            eager_overlay(imgs, maps[k], rng[k][:, 0], rng[k][:, 1], lut, 0.7)

    one_img, one_map = imgs[:1].contiguous(), maps[0, :1].contiguous()
    one_rng = ops.map_range(one_map)
    # the two routes compute the same picture (at most one level apart: the eager one rounds 1 - alpha and the blend differently)
    same = (ops.overlay_u8(one_img, one_map, one_rng, lut, 0.7).int() - eager_overlay(one_img, one_map, one_rng[:, 0], one_rng[:, 1], lut, 0.7).int()).abs().max().item()
    assert same <= 1, same
    res = {"images": n, "maps": K, "size": S, "repeats": a.repeats, "copy_rate_TBps": copy_rate / 1e12, "passes": {}}

    def report(name, us, nbytes, eager_us=None):
        rate = nbytes / (us * 1e-6)
        r = {"us": us, "bytes": nbytes, "TBps": rate / 1e12, "of_copy_rate": rate / copy_rate}
        if eager_us is not None:
            r.update(eager_us=eager_us, eager_over_kernel=eager_us / us)
        res["passes"][name] = r
        print(f"{name:16s} {us:10.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e12:6.2f} TB/s  {rate / copy_rate:5.2f} of the copy rate"
              + (f"   eager {eager_us:10.1f} us = {eager_us / us:5.1f} x" if eager_us is not None else ""), flush=True)

    print(f"copy rate {copy_rate / 1e12:.2f} TB/s (1 GiB device-to-device, {copy_us:.0f} us)")
    report("grid range", timed(k_range, a.repeats), 4 * pix * K, timed(e_range, a.repeats))
    report("grid overlay", timed(k_overlay, a.repeats), 19 * pix * K, timed(e_overlay, a.repeats))
    report("single range", timed(lambda: ops.map_range(one_map), a.repeats), 4 * S * S, timed(lambda: eager_range(one_map), a.repeats))
    report("single overlay", timed(lambda: ops.overlay_u8(one_img, one_map, one_rng, lut, 0.7), a.repeats), 19 * S * S,
           timed(lambda: eager_overlay(one_img, one_map, one_rng[:, 0], one_rng[:, 1], lut, 0.7), a.repeats))
    report("grid points", timed(lambda: ops.overlay_u8(imgs, pts=pts, colors=colors, glyphs=font, radius=radius, ring=ring, out=canvas,
                                                        cols=cols, gap=V.GAP), a.repeats), 15 * pix)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
