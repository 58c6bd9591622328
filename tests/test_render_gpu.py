"""GPU tests of keypoint visualisation: the range and overlay kernels (csrc/skp_overlay.hip) against torch and against the numpy fp64
restatement of tests/_render_cases.py, and the stage end to end on the seeded `tiny` tree."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _render_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. range
# ---------------------------------------------------------------------------------------------------------------------------------
def _range_input(N, plane, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, plane, generator=g) * 3
    if plane > 16:
        x[:, 5::7] = -0.0
        x[:, 3::11] = float("nan")
        x[:, -1] = float("nan")                                   # the last element of the last segment
    elif N > 1:
        x[0], x[1] = -0.0, float("nan")                           # plane 1: a map that is -0.0, a map that is only NaN
    else:
        x[0] = -0.0
    return x


def _range_want(x):
    nan = torch.isnan(x)
    lo = torch.where(nan, torch.full_like(x, float("inf")), x).amin(dim=1)
    hi = torch.where(nan, torch.full_like(x, float("-inf")), x).amax(dim=1)
    empty = nan.all(dim=1)
    lo[empty], hi[empty] = 0.0, 0.0
    return torch.stack([lo, hi], dim=1)


@pytest.mark.parametrize("plane", [1, 63, 64, 4097, 512 * 512])
@pytest.mark.parametrize("N", [1, 3, 33])
def test_map_range_is_bitwise_amin_amax(N, plane):
    """Negatives, -0.0 and NaN; one map over up to 256 workgroups and 33 maps at once: the bits of torch.amin / torch.amax of the
    NaN-masked input, whatever the split."""
    from stablekeypoints_amd import ops
    x = _range_input(N, plane, 100 * N + plane % 97)
    got = ops.map_range(x.cuda().view(N, 1, plane)).cpu()
    want = _range_want(x)
    assert got.shape == (N, 2) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    if plane == 1 and N > 1:
        assert got[0].view(torch.int32).tolist() == [-2 ** 31, -2 ** 31] and got[1].tolist() == [0.0, 0.0]


def test_map_range_all_nan_unaligned_and_4d():
    from stablekeypoints_amd import ops
    x = _range_input(3, 4096, 7)
    x[1] = float("nan")
    assert torch.equal(ops.map_range(x.cuda().view(3, 64, 64)).cpu().view(torch.int32), _range_want(x).view(torch.int32))
    assert ops.map_range(x.cuda().view(3, 64, 64))[1].tolist() == [0.0, 0.0]
    buf = torch.zeros(3 * 4096 + 1).cuda()                         # maps that start 4 bytes off a 16-byte boundary: the scalar form
    buf[1:] = x.reshape(-1).cuda()
    assert torch.equal(ops.map_range(buf[1:].view(3, 64, 64)).cpu().view(torch.int32), _range_want(x).view(torch.int32))
    y = _range_input(6, 256, 9)
    assert torch.equal(ops.map_range(y.cuda().view(2, 3, 16, 16)).cpu().view(torch.int32), _range_want(y).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. overlay
# ---------------------------------------------------------------------------------------------------------------------------------
def _render(case):
    """The case through `visualize.overlay` on the device -> uint8 array: [B,H,W,3], or the canvas of the case's layout."""
    from stablekeypoints_amd import visualize as V
    cu = lambda t: None if t is None else t.cuda()
    kw = dict(alpha=case["alpha"], cmap=V.VIRIDIS if case["lut"] is None else case["lut"], colors=case["colors"],
              radius=case["radius"], ring=case["ring"], labels=case["labels"])
    if case["layout"] is None:
        return V.overlay(cu(case["img"]), cu(case["maps"]), cu(case["pts"]), **kw).cpu().numpy()
    cols, gap, origin, _, _ = case["layout"]
    (h, w), _ = C.canvas_shape(case)
    canvas = torch.full((h, w, 3), C.FILL, dtype=torch.uint8).cuda()
    out = V.overlay(cu(case["img"]), cu(case["maps"]), cu(case["pts"]), out=canvas, origin=origin, cols=cols, gap=gap, **kw)
    assert out is canvas
    return canvas.cpu().numpy()


@pytest.fixture(scope="module")
def rendered():
    """Every case once: name -> (bytes from the device, expected bytes)."""
    out = {}
    for name in C.NAMES:
        case = C.build(name)
        out[name] = (_render(case), case["want"] if case["layout"] is None else C.expected_canvas(case))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_overlay_against_the_fp64_restatement(rendered, name):
    """At most one level anywhere (canvas bytes outside the tiles: untouched, so equal); the cases marked exact are exact."""
    got, want = rendered[name]
    worst, differing, n = C.compare(got, want)
    print(f"{name}: worst {worst}, {differing} of {n} bytes differ")
    assert got.shape == want.shape and worst <= 1
    case = C.build(name)
    if case["exact"]:
        assert differing == 0
    if case["layout"] is not None:
        outside = np.ones(got.shape[:2], dtype=bool)
        for y, x in C.canvas_shape(case)[1]:
            outside[y:y + case["H"], x:x + case["W"]] = False
        assert outside.any() and (got[outside] == C.FILL).all()


def test_overlay_share_of_differing_bytes(rendered):
    """Over the cases that are not asserted exact: the share of bytes that differ at all from the restatement is at most four times
    the share of `overlay_formula` in fp32 (tests/_render_cases.py)."""
    differing = total = 0
    for name in C.NAMES:
        if not C.build(name)["exact"]:
            _, d, _ = C.compare(*rendered[name])
            differing, total = differing + d, total + C.build(name)["want"].size
    print(f"kernel: {differing} of {total} bytes differ (share {differing / total:.3e}); formula fp32: {C.FORMULA_FP32_SHARE:.3e}")
    assert total == C.FORMULA_BYTES
    assert differing / total <= C.SHARE_FACTOR * C.FORMULA_FP32_SHARE


def test_plain_overlay_is_image_u8_nhwc_and_the_ledger_shows_the_kernels():
    from stablekeypoints_amd import ops, routes
    from stablekeypoints_amd import visualize as V
    g = torch.Generator().manual_seed(2)
    for shape in ((2, 3, 8, 8), (2, 3, 16, 20), (3, 3, 33, 19), (1, 3, 64, 64)):
        x = torch.rand(*shape, generator=g).cuda()
        assert torch.equal(ops.overlay_u8(x), ops.image_u8_nhwc(x))
        assert torch.equal(V.overlay(x), ops.image_u8_nhwc(x))
    routes.reset()
    before = routes.snapshot()
    x = torch.rand(2, 3, 16, 16, generator=g).cuda()
    V.overlay(x, torch.randn(2, 16, 16, generator=g).cuda(), torch.rand(2, 3, 2, generator=g).cuda())
    V.overlay(x, points=torch.rand(2, 3, 2, generator=g).cuda())
    assert routes.delta(before) == {("visualize.range", "map_range"): 1, ("visualize.overlay", "overlay_u8"): 2}
    with pytest.raises(RuntimeError, match="SKP_E_BADARG"):          # a tile outside the canvas is refused by the entry itself
        ops.overlay_u8(x, out=torch.zeros(16, 31, 3, dtype=torch.uint8).cuda(), cols=2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. end to end on the seeded tiny tree
# ---------------------------------------------------------------------------------------------------------------------------------
class _Annotated(torch.utils.data.Dataset):
    def __init__(self, data, kpts):
        self.data, self.kpts = data, kpts

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, i):
        return {"img": self.data[i], "kpts": self.kpts[i]}


def _within_one_level(path, want):
    got = C.read_png(path)
    assert got.shape == want.shape, (path, got.shape, want.shape)
    worst, differing, n = C.compare(got, want)
    print(f"{os.path.basename(path)}: worst {worst}, {differing} of {n} bytes differ")
    assert worst <= 1, path


def _grid(tiles, rows, cols, gap):
    """uint8 tiles [n,H,W,3] -> the white canvas of a rows x cols grid."""
    n, H, W, _ = tiles.shape
    canvas = np.full((rows * (H + gap) - gap, cols * (W + gap) - gap, 3), 255, dtype=np.uint8)
    for b in range(n):
        y, x = (b // cols) * (H + gap), (b % cols) * (W + gap)
        canvas[y:y + H, x:x + W] = tiles[b]
    return canvas


def test_visualize_attn_maps_end_to_end(tmp_path):
    """128^2 synthetic images, 4 tokens, 2 views, a 2 x 3 grid with injected draws: the expected files, each within one level of the
    restatement rendered from the returned points and the maps of a second augmented-inference call with the same draws."""
    from stablekeypoints_amd import visualize as V
    from stablekeypoints_amd.eval import run_images_with_context_augmented
    from stablekeypoints_amd.invertable_transform import RandomAffineWithInverse
    from stablekeypoints_amd.optimize import SyntheticImages, default_args
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, n_gpus = load_ldm("cuda", "tiny", feature_upsample_res=32)
    g = torch.Generator().manual_seed(21)
    T, K, n, views = 16, 4, 6, 2
    ctx = torch.randn(1, T, 768, generator=g).cuda()
    idx = torch.tensor([3, 7, 1, 12])
    images = SyntheticImages(n=4, size=128, seed=5, device="cuda").data
    data = _Annotated(images, torch.rand(4, 3, 2, generator=g))
    args = default_args(num_tokens=T, top_k=K, augmentation_iterations=views, images_per_forward=4, save_folder=str(tmp_path / "out"),
                        feature_upsample_res=32)
    order = [2, 0, 3, 1]
    noise = torch.randn(n * views, 4, 16, 16, generator=g)
    torch.manual_seed(4)
    thetas = RandomAffineWithInverse(degrees=args.augment_degrees, scale=args.augment_scale,
                                     translate=args.augment_translate).sample_theta(n * views)
    points, files = V.visualize_attn_maps(ldm, ctx, idx, args, controllers, n_gpus, regressor=torch.eye(2 * K), height=2, width=3,
                                          dataset=data, draws=(order, noise, thetas))
    names = ["unsupervised_keypoints.png"] + [f"keypoint_{k:03d}.png" for k in range(K)] + ["estimated_keypoints.png", "gt_keypoints.png"]
    assert [os.path.basename(f) for f in files] == names and all(os.path.isfile(f) for f in files)
    assert points.shape == (n, K, 2) and float(points.min()) >= 0 and float(points.max()) <= 1
    shown = torch.stack([images[order[i % 4]] for i in range(n)])
    maps = run_images_with_context_augmented(ldm, shown, ctx, idx, controllers=controllers, layers=args.layers,
                                             augmentation_iterations=views, noise_level=args.noise_level,
                                             augment_degrees=args.augment_degrees, augment_scale=args.augment_scale,
                                             augment_translate=args.augment_translate, num_gpus=n_gpus, upscale_size=512,
                                             thetas=thetas, noise=noise)
    assert maps.shape == (n, K, 512, 512)
    shown, maps = shown.cpu().numpy(), maps.cpu().numpy()
    radius, ring = V.marker_size(128)
    kw = dict(lut=V.VIRIDIS.numpy(), glyphs=V.FONT_5X7.numpy(), alpha=0.7, radius=radius, ring=ring, labels=True)
    folder = str(tmp_path / "out")
    for name, pts in (("unsupervised_keypoints.png", points), ("estimated_keypoints.png", points),
                      ("gt_keypoints.png", torch.stack([data.kpts[order[i % 4]] for i in range(n)]))):
        tiles = C.to_bytes(C.restate(shown, None, pts.numpy(), colors=V.cycle_colors(pts.shape[1]).numpy(), **kw))
        _within_one_level(os.path.join(folder, name), _grid(tiles, 2, 3, V.GAP))
    plain = C.to_bytes(C.restate(shown, None, None, colors=None, **kw))
    for k in range(K):
        heat = C.to_bytes(C.restate(shown, maps[:, k], None, colors=None, **kw))
        _within_one_level(os.path.join(folder, f"keypoint_{k:03d}.png"), _grid(np.concatenate([plain, heat]), 2, n, V.GAP))


def test_find_keypoints_tool(tmp_path, monkeypatch):
    """tools/find_keypoints.main on a folder of four images: every stage's files, K in-range pairs per image, and the same
    keypoints.json from a second run that is handed the embedding and the indices of the first."""
    pytest.importorskip("PIL")
    from stablekeypoints_amd import visualize as V
    spec = importlib.util.spec_from_file_location("find_keypoints", os.path.join(ROOT, "tools", "find_keypoints.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setenv("SKP_ALLOW_SYNTHETIC", "1")
    src = tmp_path / "images"
    src.mkdir()
    px = np.random.RandomState(8).randint(0, 256, size=(4, 128, 128, 3)).astype(np.uint8)
    stems = ["b", "a", "d", "c"]
    for i, s in enumerate(stems):
        V.write_png(str(src / f"{s}.png"), px[i])
    K = 4
    common = ["--model", "tiny", "--images", str(src), "--image-size", "128", "--feature-upsample-res", "32", "--num-steps", "2",
              "--num-tokens", "16", "--num-indices", "4", "--top-k", str(K), "--augmentation-iterations", "2",
              "--images-per-forward", "4", "--grid", "2", "3", "--seed", "3"]
    first = str(tmp_path / "first")
    files = tool.main(common + ["--out", first])
    want = ["embedding.pt", "indices.pt", "keypoints.json", "keypoints.pt"] + [f"{s}_keypoints.png" for s in sorted(stems)] + \
           ["unsupervised_keypoints.png"] + [f"keypoint_{k:03d}.png" for k in range(K)]
    assert [os.path.basename(f) for f in files] == want and all(os.path.isfile(os.path.join(first, f)) for f in want)
    kp = json.load(open(os.path.join(first, "keypoints.json")))
    assert list(kp) == [f"{s}.png" for s in sorted(stems)]
    for pairs in kp.values():
        assert len(pairs) == K and all(len(p) == 2 and 0 <= p[0] <= 1 and 0 <= p[1] <= 1 for p in pairs)
    assert torch.equal(torch.load(os.path.join(first, "keypoints.pt")), torch.tensor(list(kp.values())))
    assert tuple(torch.load(os.path.join(first, "embedding.pt")).shape) == (1, 16, 768)
    assert tuple(torch.load(os.path.join(first, "indices.pt")).shape) == (K,)
    assert C.read_png(os.path.join(first, "a_keypoints.png")).shape == (128, 128, 3)
    assert C.read_png(os.path.join(first, "unsupervised_keypoints.png")).shape == (2 * 128 + V.GAP, 3 * 128 + 2 * V.GAP, 3)
    assert C.read_png(os.path.join(first, "keypoint_000.png")).shape == (2 * 128 + V.GAP, 6 * 128 + 5 * V.GAP, 3)
    second = str(tmp_path / "second")
    tool.main(common + ["--out", second, "--embedding", os.path.join(first, "embedding.pt"), "--indices", os.path.join(first, "indices.pt")])
    assert json.load(open(os.path.join(second, "keypoints.json"))) == kp
