"""GPU tests of the evaluation stage on the seeded `tiny` tree: `precompute_all_keypoints(batched_locator=True)` against the per-image
path, and `eval.evaluate` end to end on a six-image annotated dataset with injected draws."""
import numpy as np
import pytest
import torch

import _locate_cases as C
from oracle import ref_path as R
from oracle.fixtures import seeded

pytestmark = pytest.mark.gpu

SIZE, N_IMAGES, N_AUG, GROUP, T, RES = 128, 6, 2, 4, 16, 32
INDICES = [1, 5, 9, 12]


class _Annotated(torch.utils.data.Dataset):
    def __init__(self):
        g = torch.Generator().manual_seed(141)
        self.img = torch.rand(N_IMAGES, 3, SIZE, SIZE, generator=g)
        self.kpts = torch.rand(N_IMAGES, 3, 2, generator=g) * 0.8 + 0.1
        self.vis = (torch.rand(N_IMAGES, 3, generator=g) > 0.3).float()
        self.vis[:, 0] = 1

    def __len__(self):
        return N_IMAGES

    def __getitem__(self, i):
        return {"img": self.img[i], "kpts": self.kpts[i], "visibility": self.vis[i]}


def _draws():
    g = torch.Generator().manual_seed(142)
    n = N_IMAGES * N_AUG
    u = torch.rand(n, 4, generator=g)
    thetas = torch.cat([R.affine_matrix(float(30 * a - 15), float(0.8 + 0.2 * s), (float(0.5 * x - 0.25), float(0.5 * y - 0.25)))
                        for a, s, x, y in u.tolist()])
    return [3, 0, 5, 1, 4, 2], torch.randn(n, 4, SIZE // 8, SIZE // 8, generator=g), thetas


def _args(strategy, **over):
    from stablekeypoints_amd.optimize import default_args
    return default_args(num_tokens=T, feature_upsample_res=RES, image_size=SIZE, device="cuda", augmentation_iterations=N_AUG,
                        images_per_forward=GROUP, max_loc_strategy=strategy, max_num_points=50_000, **over)


@pytest.fixture(scope="module")
def tiny():
    """The seeded tree; the convolution library's deterministic algorithms for the length of the module, as tools/find_keypoints.py
    asks for them: the tests compare two runs of the same inference bit for bit."""
    from stablekeypoints_amd.optimize_token import load_ldm
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    ldm, controllers, n = load_ldm("cuda", "tiny", feature_upsample_res=RES)
    yield ldm, controllers, n, (seeded((1, T, 768), 143)).cuda()
    torch.backends.cudnn.deterministic = before


def test_batched_locator_is_the_per_image_path(tiny):
    """One locator launch per group against `keypoints_from_maps` per image, same draws: the arg-max locations are equal bit for bit;
    the weighted locations agree within the locator's tolerance (4 x the measured fp32 error of the reference's op order, in pixels
    of the 512-pixel maps, over 512); the annotations pass through alike; the ledger counts one launch per group."""
    from stablekeypoints_amd import routes
    from stablekeypoints_amd.keypoint_regressor import precompute_all_keypoints
    ldm, controllers, n, ctx = tiny
    ds, idx = _Annotated(), torch.tensor(INDICES)
    for strategy in ("argmax", "weighted_avg"):
        one = precompute_all_keypoints(ldm, ctx, idx, _args(strategy), controllers, n, dataset=ds, draws=_draws())
        many = precompute_all_keypoints(ldm, ctx, idx, _args(strategy), controllers, n, dataset=ds, draws=_draws(), routes="report",
                                        batched_locator=True)
        assert routes.snapshot()[("eval.locate", "locate")] == -(-N_IMAGES // GROUP)
        assert many[0].shape == (N_IMAGES, len(INDICES), 2) and many[0].dtype == one[0].dtype and many[0].device == one[0].device
        assert torch.equal(many[1], one[1]) and torch.equal(many[2], one[2]) and torch.equal(many[1], ds.kpts[_draws()[0]])
        diff = float((many[0] - one[0]).abs().max())
        print(f"{strategy}: batched vs per image, max |diff| {diff:.3e} of the map side")
        if strategy == "argmax":
            assert torch.equal(many[0], one[0])
        else:
            assert diff <= C.tolerance(5) / 512
            assert not torch.equal(many[0] * 512 % 1, torch.full_like(many[0], 0.5))             # (not pixel centres)


@pytest.mark.parametrize("method", ["mean_average_error", "inter_eye_distance"])
def test_evaluate_end_to_end(tiny, tmp_path, monkeypatch, method):
    """`evaluate` = the dataset loop with the batched locator + `keypoint_errors`: what it returns is `keypoint_errors` of the
    locations the loop found (which are `precompute_all_keypoints(batched_locator=True)`'s for the same draws), in the order of the
    draws; all_errors.pt holds it; the ledger shows one locator launch per group; `routes="strict"` passes.
    (Strict runs inside `ops.conv3x3_own_kernels()`: at 128^2 images the reduced tree's 4^2 level has too few tiles for
    `conv3x3_plan`'s tile rule and goes to the library, with or without the evaluation stage, which plain strict refuses -- the
    reason tests/test_routes_gpu.py pins strict at 512^2 and 16 rows.  With the tile rule dropped every convolution stays on the
    HIP kernels and the strict rule covers what `evaluate` adds: the locator, and nothing outside the kernels.)"""
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd import ops, routes
    from stablekeypoints_amd.keypoint_regressor import precompute_all_keypoints, return_regressor
    ldm, controllers, n, ctx = tiny
    ds, idx = _Annotated(), torch.tensor(INDICES)
    args = _args("argmax", evaluation_method=method, save_folder=str(tmp_path / "out"))
    src, tgt, vis = precompute_all_keypoints(ldm, ctx, idx, args, controllers, n, dataset=ds, draws=_draws(), batched_locator=True)
    W = torch.tensor(return_regressor(src.reshape(N_IMAGES, -1).cpu(), tgt.reshape(N_IMAGES, -1))).float().cuda()
    seen, real = [], E.keypoint_errors

    def spy(*a, **k):
        seen.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(E, "keypoint_errors", spy)
    mean, errors = E.evaluate(ldm, ctx, idx, W, args, controllers, n, dataset=ds, draws=_draws(), routes="report")
    assert routes.snapshot()[("eval.locate", "locate")] == -(-N_IMAGES // GROUP)
    assert len(seen) == 1 and torch.equal(seen[0][0][0], src)                                  # the same locations
    want = real(src, W, tgt.cuda(), vis, method).cpu()
    assert tuple(errors.shape) == (N_IMAGES,) and not errors.is_cuda and torch.equal(errors, want)
    assert mean == float(want.mean()) and np.isfinite(mean) and mean > 0
    assert torch.equal(torch.load(str(tmp_path / "out" / "all_errors.pt")), errors)
    # without draws: dataset order, every image; strict routes
    with ops.conv3x3_own_kernels():
        mean2, errors2 = E.evaluate(ldm, ctx, idx, W, _args("weighted_avg", evaluation_method=method), controllers, n, dataset=ds,
                                    routes="strict")
    snap = routes.snapshot()
    assert snap[("eval.locate", "locate")] == -(-N_IMAGES // GROUP)
    assert all(routes.kind(s, r) == "hip" or (s, r) in routes.DOCUMENTED_LIBRARY_ROUTES for s, r in snap)
    assert tuple(errors2.shape) == (N_IMAGES,) and torch.isfinite(errors2).all()
    assert torch.equal(seen[-1][0][2].cpu(), ds.kpts)
    with pytest.raises(ValueError, match="evaluation method"):
        E.evaluate(ldm, ctx, idx, W, _args("argmax", evaluation_method="mean"), controllers, n, dataset=ds)
