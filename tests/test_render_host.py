"""CPU tests of keypoint visualisation (stablekeypoints_amd/visualize.py): the overlay header against its table, refusals before any
launch, the torch formula against the numpy fp64 restatement of tests/_render_cases.py, the glyph table, the PNG writer and the
grids on host tensors."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _render_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["skp_map_range_f32", "skp_map_range_workspace", "skp_overlay_u8_f32"]


def _host_logic():
    spec = importlib.util.spec_from_file_location("_host_logic", os.path.join(ROOT, "tests", "test_host_logic.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the C entries
# ---------------------------------------------------------------------------------------------------------------------------------
def test_overlay_header_agrees_with_its_table():
    """include/skp_overlay.h against `_native.OVERLAY_SIGNATURES` with the comparison tests/test_host_logic.py applies to skp.h; the
    library exports the entries, the table is disjoint from the other two, the launching entries end in the stream, the ABI moved."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    H = _host_logic()
    hdr = open(os.path.join(ROOT, "include", "skp_overlay.h")).read()
    abi = H._header_abi(hdr)
    assert sorted(abi) == sorted(N.OVERLAY_SIGNATURES) == ENTRIES
    assert H._abi_mismatches(hdr, N.OVERLAY_SIGNATURES) == []
    assert not set(N.OVERLAY_SIGNATURES) & (set(N.SIGNATURES) | set(N.KEYPOINT_SIGNATURES))
    for name in ("skp_map_range_f32", "skp_overlay_u8_f32"):
        assert abi[name][1][-1] == "dev:void" and N.signature(name) is N.OVERLAY_SIGNATURES[name]
    lib = N.lib()
    assert lib.skp_abi_version() == N.ABI_VERSION >= 46
    for name, argtypes in N.OVERLAY_SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    assert len(ops._plan("skp_overlay_u8_f32")[1]) == len(N.OVERLAY_SIGNATURES["skp_overlay_u8_f32"]) - 1
    mk = open(os.path.join(ROOT, "stablekeypoints_amd", "csrc", "Makefile")).read()
    assert "skp_overlay.hip" in mk and "skp_overlay.h" in mk


def _overlay_args(**over):
    """A legal argument list of skp_overlay_u8_f32 (any non-null address: arguments are refused before a launch), edited by name."""
    one = 16
    a = dict(img=one, map=one, range=one, lut=one, pts=one, colors=one, glyphs=one, out=one, B=2, H=8, W=8, S=8, L=9, K=3, alpha=0.7,
             radius=3.0, ring=1.0, labels=1, ld=8, canvas_h=16, y0=0, x0=0, cols=1, gap=0)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values()) + [None]


def test_entries_refuse_bad_arguments_before_launching():
    from stablekeypoints_amd import _native as N
    lib = N.lib()
    one = 16
    BAD, RANGE = -1, -2
    assert lib.skp_map_range_workspace(0, 64) == BAD and lib.skp_map_range_workspace(3, 0) == BAD
    assert lib.skp_map_range_workspace(990, 512 * 512) > 0 and lib.skp_map_range_workspace(1, 512 * 512) > 0
    assert lib.skp_map_range_workspace(5000, 4096) == 0 and lib.skp_map_range_workspace(1, 63) == 0
    assert lib.skp_map_range_f32(None, one, one, 1, 64, None) == BAD
    assert lib.skp_map_range_f32(one, None, one, 1, 64, None) == BAD
    assert lib.skp_map_range_f32(one, one, one, 0, 64, None) == BAD
    assert lib.skp_map_range_f32(one, one, one, 1, 0, None) == BAD
    assert lib.skp_map_range_f32(one, one, None, 1, 512 * 512, None) == BAD            # the query asks for scratch here
    ov = lib.skp_overlay_u8_f32
    for name in ("img", "out", "range", "lut", "pts", "colors", "glyphs"):
        assert ov(*_overlay_args(**{name: None})) == BAD, name
    for name in ("B", "H", "W", "S"):
        for v in (0, -1):
            assert ov(*_overlay_args(**{name: v})) == BAD, name
    assert ov(*_overlay_args(L=1)) == BAD and ov(*_overlay_args(K=-1)) == BAD
    assert ov(*_overlay_args(radius=-1.0)) == BAD and ov(*_overlay_args(ring=float("nan"))) == BAD
    assert ov(*_overlay_args(cols=0)) == BAD and ov(*_overlay_args(gap=-1)) == BAD and ov(*_overlay_args(x0=-1)) == BAD
    assert ov(*_overlay_args(ld=7)) == BAD and ov(*_overlay_args(canvas_h=15)) == BAD           # a tile outside the canvas
    assert ov(*_overlay_args(cols=2, ld=17, gap=2)) == BAD and ov(*_overlay_args(y0=1)) == BAD
    assert ov(*_overlay_args(K=101)) == RANGE and ov(*_overlay_args(L=1025)) == RANGE
    assert ov(*_overlay_args(H=4097, canvas_h=2 * 4097)) == RANGE and ov(*_overlay_args(W=4097, ld=4097)) == RANGE
    assert ov(*_overlay_args(S=4097)) == RANGE


def test_ops_have_no_cpu_fallback_and_routes_are_registered():
    from stablekeypoints_amd import ops, routes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.map_range(torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.overlay_u8(torch.zeros(1, 3, 4, 4))
    assert routes.ROUTES["visualize.range"] == {"map_range": "hip", "host": "host"}
    assert routes.ROUTES["visualize.overlay"] == {"overlay_u8": "hip", "host": "host"}


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the formula
# ---------------------------------------------------------------------------------------------------------------------------------
def _formula(case, dtype):
    from stablekeypoints_amd import visualize as V
    cast = lambda t: None if t is None else t.to(dtype)
    return V.overlay_formula(cast(case["img"]), cast(case["maps"]), cast(case["pts"]), alpha=case["alpha"],
                             cmap=V.VIRIDIS if case["lut"] is None else case["lut"], colors=case["colors"], radius=case["radius"],
                             ring=case["ring"], labels=case["labels"]).numpy()


@pytest.mark.parametrize("name", C.NAMES)
def test_formula_fp64_is_the_restatement(name):
    """`overlay_formula` in fp64 against the numpy restatement: exact bytes, every case."""
    case = C.build(name)
    worst, differing, _ = C.compare(_formula(case, torch.float64), case["want"])
    assert (worst, differing) == (0, 0)


def test_formula_fp32_within_one_level():
    """`overlay_formula` in fp32 against the same restatement: at most one level anywhere, the exact cases exact; the share of
    differing bytes of the other cases is what tests/_render_cases.py records (the GPU test's cap is four times it)."""
    differing = total = 0
    for name in C.NAMES:
        case = C.build(name)
        worst, d, n = C.compare(_formula(case, torch.float32), case["want"])
        print(f"{name}: worst {worst}, {d} of {n} bytes differ")
        assert worst <= 1, name
        if case["exact"]:
            assert d == 0, name
        else:
            differing, total = differing + d, total + n
    print(f"fp32 formula: {differing} of {total} bytes differ (share {differing / total:.3e})")
    assert (differing, total) == (C.FORMULA_FP32_DIFFERING, C.FORMULA_BYTES)


def test_the_cases_reach_what_they_name():
    """The generator's guards held, and the marker cases paint what they say: two overlapping markers, digits, NaN points."""
    from stablekeypoints_amd import visualize as V
    case = C.build("markers only K 12 big")
    pts = case["pts"].numpy()
    assert np.isnan(pts[0, 7]).all() and np.isnan(pts[-1, 8, 1])
    assert min(pts[0, :4, :].min(), 1 - pts[0, :4, :].max()) < 0.01
    assert np.abs(pts[0, 6] - pts[0, 5]).max() < 0.05                       # markers 5 and 6 overlap (radius 9 of 64 pixels)
    no_labels = C.to_bytes(C.restate(case["img"].numpy(), None, pts, lut=None, colors=case["colors"].numpy(),
                                     glyphs=V.FONT_5X7.numpy(), alpha=0.7, radius=9.0, ring=1.5, labels=False))
    assert (no_labels != case["want"]).any(axis=-1).sum() > 12 * 7                               # the digits are pixels
    assert V.glyph_scale(9.0, 1) == C.glyph_scale(9.0, 1) == 2 and V.glyph_scale(9.0, 2) == 1 and V.glyph_scale(3.0, 1) == 1
    assert V.marker_size(512) == (9.0, 1.5) and V.marker_size(64) == (3.0, 1.0)


def test_glyph_table():
    from stablekeypoints_amd import visualize as V
    g = V.FONT_5X7
    assert g.dtype == torch.uint8 and tuple(g.shape) == (10, 7) and int(g.max()) < 32
    assert len({tuple(r) for r in g.tolist()}) == 10 and all(sum(r) > 0 for r in g.tolist())
    assert V.VIRIDIS.shape[0] >= 9 and V.VIRIDIS.shape[1] == 3 and tuple(V.COLORS.shape) == (10, 3)
    assert 0 <= float(V.VIRIDIS.min()) and float(V.VIRIDIS.max()) <= 1 and 0 <= float(V.COLORS.min()) and float(V.COLORS.max()) <= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. files and grids
# ---------------------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trip(tmp_path):
    from stablekeypoints_amd import visualize as V
    px = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(13, 21, 3)).astype(np.uint8))
    path = V.write_png(str(tmp_path / "a.png"), px)
    assert np.array_equal(C.read_png(path), px.numpy())
    assert np.array_equal(C.read_png(V.write_png(str(tmp_path / "b.png"), px.numpy())), px.numpy())
    with pytest.raises(ValueError):
        V.write_png(str(tmp_path / "c.png"), px.float())
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), px.numpy())


def test_grids_on_host_tensors(tmp_path):
    """`save_grid` / `plot_point_correspondences` / `plot_point_single` on CPU tensors: canvas size, tile positions, gaps and an
    absent tile stay 255, the files hold the canvas, and the ledger shows the host routes."""
    from stablekeypoints_amd import routes
    from stablekeypoints_amd import visualize as V
    g = torch.Generator().manual_seed(5)
    H = W = 16
    imgs = torch.rand(5, 3, H, W, generator=g)
    maps = torch.randn(5, 8, 8, generator=g)
    pts = torch.rand(5, 3, 2, generator=g)
    gap = V.GAP
    before = routes.snapshot()
    grid = V.save_grid(maps[:3], list(imgs[:3]), str(tmp_path / "grid.png"))
    assert routes.delta(before) == {("visualize.overlay", "host"): 2, ("visualize.range", "host"): 1}
    assert tuple(grid.shape) == (2 * H + gap, 3 * W + 2 * gap, 3) and np.array_equal(C.read_png(str(tmp_path / "grid.png")), grid.numpy())
    plain, heat = V.overlay_formula(imgs[:3]), V.overlay_formula(imgs[:3], maps[:3])
    for b in range(3):
        x = b * (W + gap)
        assert torch.equal(grid[:H, x:x + W], plain[b]) and torch.equal(grid[H + gap:, x:x + W], heat[b])
    assert (grid[H:H + gap] == 255).all() and (grid[:, W:W + gap] == 255).all() and (grid[:, 2 * W + gap:2 * W + 2 * gap] == 255).all()
    # 5 images into a 2 x 3 grid: the sixth tile stays white
    grid = V.plot_point_correspondences(imgs, pts, str(tmp_path / "points.png"), height=2, width=3)
    assert tuple(grid.shape) == (2 * H + gap, 3 * W + 2 * gap, 3) and np.array_equal(C.read_png(str(tmp_path / "points.png")), grid.numpy())
    marked = V.overlay_formula(imgs, points=pts)
    for b in range(5):
        y, x = (b // 3) * (H + gap), (b % 3) * (W + gap)
        assert torch.equal(grid[y:y + H, x:x + W], marked[b])
    assert (grid[H + gap:, 2 * (W + gap):] == 255).all() and (grid[H:H + gap] == 255).all()
    assert not torch.equal(marked, V.overlay_formula(imgs))
    # more images than tiles: the first height * width
    assert torch.equal(V.plot_point_correspondences(imgs, pts, str(tmp_path / "few.png"), height=1, width=2)[:, :W], marked[0])
    one = V.plot_point_single(imgs[0], pts[:2], str(tmp_path / "one.png"))
    assert tuple(one.shape) == (H, W, 3) and np.array_equal(C.read_png(str(tmp_path / "one.png")), one.numpy())
    first = V.overlay_formula(imgs[:1], points=pts[:1])
    again = V.overlay_formula((first.permute(0, 3, 1, 2).float() + 0.5) / 255, points=pts[1:2])[0]
    assert torch.equal(one, again) and not torch.equal(one, first[0])
    # the overlay refuses a tile outside a host canvas, and more points than two digits number
    with pytest.raises(ValueError):
        V.overlay(imgs[:2], out=torch.zeros(H, 2 * W - 1, 3, dtype=torch.uint8), cols=2)
    with pytest.raises(ValueError):
        V.overlay(imgs[:1], points=torch.rand(1, 101, 2))
