#!/usr/bin/env python
"""Which kernel route every gated site takes: one forward + backward group step of a synthetic model on the GPU, then the route
ledger (stablekeypoints_amd/routes.py) as a table, and the routes that are not HIP kernels with their documented reason.

    python tools/routes_report.py --arch sd15|sd21|sdxl [--size 512] [--rows 8] [--tiny] [--tokens 77] [--res 128]

`--rows`: batch rows of the step (images x 2 views).  `--tiny`: the reduced-width tree of the architecture.  Exit status 1 if a
route outside the HIP kernels ran that `routes.DOCUMENTED_LIBRARY_ROUTES` does not list.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_SIZE = {"sd15": 512, "sd21": 768, "sdxl": 1024}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", choices=sorted(DEFAULT_SIZE), default="sd15")
    ap.add_argument("--size", type=int, default=0, help="image side (default: 512 / 768 / 1024 by architecture)")
    ap.add_argument("--rows", type=int, default=8, help="batch rows of the step = 2 x images")
    ap.add_argument("--tiny", action="store_true", help="reduced-width tree")
    ap.add_argument("--tokens", type=int, default=77)
    ap.add_argument("--res", type=int, default=128, help="feature_upsample_res")
    a = ap.parse_args()
    if a.rows < 2 or a.rows % 2:
        ap.error("--rows must be an even number >= 2 (every image goes through with its affine copy)")
    import torch
    if not torch.cuda.is_available():
        print("routes_report: needs the GPU", file=sys.stderr)
        return 2
    from stablekeypoints_amd import routes
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    from stablekeypoints_amd.optimize import default_args, group_step
    from stablekeypoints_amd.optimize_token import load_ldm
    size = a.size or DEFAULT_SIZE[a.arch]
    name = ("tiny" if a.arch == "sd15" else f"tiny-{a.arch}") if a.tiny else a.arch
    ldm, controllers, _ = load_ldm("cuda", name, feature_upsample_res=a.res, init_on_device=True)
    dev, controller = next(iter(controllers.items()))
    n = a.rows // 2
    g = torch.Generator().manual_seed(0)
    images = torch.rand(n, 3, size, size, generator=g)
    ctx = (torch.randn(1, a.tokens, ldm.unet.config.get("cross_attention_dim", 768), generator=g) * 5.0).cuda().requires_grad_(True)
    args = default_args(num_tokens=a.tokens, feature_upsample_res=a.res, batch_size=n, device="cuda")
    routes.reset()
    group_step(ldm, images, ctx, args, controller, RandomAffineWithInverse(), denom=n)
    torch.cuda.synchronize()
    print(f"# {name} {size}^2, {a.rows} rows, T = {a.tokens}, R = {a.res}: one group step (forward + backward)")
    print(routes.table())
    bad = 0
    print("\nroutes outside the HIP kernels:")
    rows = routes.non_hip()
    for site, route, count, kind, reason in rows:
        print(f"  {site}/{route} x{count} [{kind}]: {reason or 'UNDOCUMENTED'}")
        bad += reason is None
    if not rows:
        print("  (none)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
