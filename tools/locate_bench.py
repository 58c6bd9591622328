#!/usr/bin/env python
"""The keypoint locator (ops.locate, csrc/skp_locate.hip: one launch for a whole group's maps) against what it replaces, the
per-image `keypoint_regressor.keypoints_from_maps` composition (one token-statistics launch per image; under `weighted_avg` the
reference's elementwise passes in eager torch on top, on a clone, since they zero their input), on the device, in one run:
    python tools/locate_bench.py [--images 4] [--maps 10] [--size 512] [--repeats 50] [--json FILE]
Per strategy: microseconds per group (median of `--repeats` after 3 warm-up rounds, device events around the whole pass, the two
routes alternating), the bytes the pass has to read (4 per pixel), and the locator's rate.  The 10 MB of a [4,10,512,512] group fit
the last-level cache: the rate is a cache rate, and most of the time of so small a pass is launch latency."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def timed_pair(f, g, repeats, warmup=3):
    """Median microseconds of f() and of g(), alternating."""
    for _ in range(warmup):
        f()
        g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(repeats):
        tf.append(once(f))
        tg.append(once(g))
    return sorted(tf)[len(tf) // 2], sorted(tg)[len(tg) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--maps", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--json")
    a = ap.parse_args(argv)
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd.keypoint_regressor import keypoints_from_maps
    assert torch.cuda.is_available(), "locate_bench.py measures on the GPU; there is nothing to measure without one"
    m, K, S = a.images, a.maps, a.size
    g = torch.Generator().manual_seed(0)
    maps = torch.rand(m, K, S, S, generator=g).cuda() ** 8          # peaked, non-negative, as averaged attention maps are
    res = {"images": m, "maps": K, "size": S, "repeats": a.repeats, "bytes": 4 * maps.numel(), "strategies": {}}
    for strategy in E.STRATEGIES:
        def batched():
            return E.locate_keypoints(maps, strategy) / float(S)

        def per_image():
            return torch.stack([keypoints_from_maps(maps[i] if strategy == "argmax" else maps[i].clone(), strategy) for i in range(m)])
        diff = float((batched() - per_image()).abs().max())
        assert diff <= (0.0 if strategy == "argmax" else 1e-6), (strategy, diff)
        us, us_old = timed_pair(batched, per_image, a.repeats)
        res["strategies"][strategy] = {"locator_us": us, "per_image_us": us_old, "per_image_over_locator": us_old / us,
                                       "locator_GBps": res["bytes"] / (us * 1e-6) / 1e9, "max_abs_diff": diff}
        print(f"{strategy:13s} locator {us:9.1f} us ({res['bytes'] / (us * 1e-6) / 1e9:7.1f} GB/s)   per image {us_old:9.1f} us = "
              f"{us_old / us:5.1f} x   max |diff| {diff:.2e} of the side", flush=True)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
