"""CPU tests of the evaluation stage: the regressors and `swap_points` against the REFERENCE's own outputs
(tests/golden/g14_reference_regressors.npz, written by tools/gen_eval_golden.py from the seeded inputs of tests/_evaluate_cases.py),
`keypoint_errors` against a numpy restatement per method, the annotated-folder dataset, and the untouched default of
`precompute_all_keypoints`."""
import inspect
import json

import numpy as np
import pytest
import torch

import _evaluate_cases as EC


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. regressors
# ---------------------------------------------------------------------------------------------------------------------------------
def _case(golden, kind):
    g = golden("g14_reference_regressors.npz")
    n, k, gg, seed = (int(v) for v in g[kind + "/spec"])
    return g, EC.regressor_inputs(kind, n, k, gg, seed)


def test_fixture_holds_what_the_tests_need(golden):
    g = golden("g14_reference_regressors.npz")
    assert {k.split("/")[0] for k in g} == set(EC.KINDS) | {"swap"}
    _, (X, _, _) = _case(golden, "deficient")
    assert np.linalg.matrix_rank((X - 0.5).T @ (X - 0.5)) < X.shape[1]                      # pinv matters
    _, (X, _, visible) = _case(golden, "visible")
    assert 0 < visible[:, 2].sum() < X.shape[1] and visible[:, 0].sum() > X.shape[1]       # a column seen in fewer rows than X has columns
    _, (_, Y, _) = _case(golden, "h36m")
    assert Y.shape[1] == 64 and 2 <= int(g["h36m/passes"]) < 10


@pytest.mark.parametrize("kind", ["plain", "deficient"])
def test_return_regressor_is_the_references(golden, kind):
    from stablekeypoints_amd.keypoint_regressor import return_regressor
    g, (X, Y, _) = _case(golden, kind)
    kx, ky = X.copy(), Y.copy()
    W = return_regressor(X, Y)
    assert W.dtype == np.float64
    np.testing.assert_allclose(W, g[kind + "/W"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(X, kx) and np.array_equal(Y, ky)
    W32 = return_regressor(torch.from_numpy(X).float(), torch.from_numpy(Y).float())           # tensors, any dtype: fitted in fp64
    assert W32.dtype == np.float64 and np.abs(W32 - W).max() < 1e-3
    if kind == "plain":                                                                        # the fit predicts the annotations
        assert np.abs((X - 0.5) @ W + 0.5 - Y).max() < 0.05


def test_return_regressor_visible_is_the_references(golden):
    from stablekeypoints_amd.keypoint_regressor import return_regressor, return_regressor_visible
    g, (X, Y, visible) = _case(golden, "visible")
    ky, kv = Y.copy(), visible.copy()
    W = return_regressor_visible(X, Y, visible)
    np.testing.assert_allclose(W, g["visible/W"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(Y, ky) and np.array_equal(visible, kv)
    np.testing.assert_allclose(return_regressor_visible(X, Y, np.ones_like(visible)), return_regressor(X, Y), rtol=1e-9, atol=1e-12)


def test_return_regressor_human36m_is_the_references(golden, monkeypatch):
    from stablekeypoints_amd import eval as E
    from stablekeypoints_amd.keypoint_regressor import return_regressor, return_regressor_human36m
    g, (X, Y, _) = _case(golden, "h36m")
    ky = Y.copy()
    passes, real = [0], E.swap_points

    def counting(points):
        passes[0] += 1
        return real(points)
    monkeypatch.setattr(E, "swap_points", counting)
    W = return_regressor_human36m(X, Y)
    np.testing.assert_allclose(W, g["h36m/W"], rtol=1e-9, atol=1e-12)
    assert passes[0] == int(g["h36m/passes"]) >= 2                    # at least one pass swapped more than 10 rows
    assert np.array_equal(Y, ky)                                      # the swaps stay inside
    assert np.abs(W - return_regressor(X, Y)).max() > 1e-3            # and they changed the fit


def test_swap_points_is_the_references(golden):
    from stablekeypoints_amd.eval import swap_points
    g = golden("g14_reference_regressors.npz")
    pts = EC.swap_input(int(g["swap/seed"]))
    keep = pts.clone()
    out = swap_points(pts)
    assert np.array_equal(out.numpy(), g["swap/out"]) and torch.equal(pts, keep)
    # the reference's list as written: after (20, 28), (21, 28) -- joint 28 ends up taking 21, and 20 and 21 both take 28
    assert torch.equal(out[:, 28], pts[:, 21]) and torch.equal(out[:, 20], pts[:, 28]) and torch.equal(out[:, 21], pts[:, 28])
    assert torch.equal(out[:, 0], pts[:, 0]) and torch.equal(out[:, 1], pts[:, 6]) and torch.equal(out[:, 31], pts[:, 23])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. metrics
# ---------------------------------------------------------------------------------------------------------------------------------
def _errors_numpy(loc, W, gt, vis, method):
    """eval.py:452-494, image by image, in numpy fp64."""
    out = []
    for i in range(loc.shape[0]):
        est = ((loc[i].reshape(1, -1) - 0.5) @ W + 0.5).reshape(-1, 2)
        g = gt[i].copy()
        if method in ("mean_average_error", "pck"):
            est, g = est * 256, g * 256
        l2 = np.sqrt(((est - g) ** 2).sum(-1))
        v = np.ones_like(l2) if vis is None else vis[i]
        if method == "inter_eye_distance":
            e = (l2 / np.sqrt(((g[0] - g[1]) ** 2).sum())).mean()
        elif method == "visible":
            with np.errstate(invalid="ignore"):
                e = (l2 * v).sum() / v.sum()
        elif method == "mean_average_error":
            e = (l2 * v).sum()
        elif method == "pck":
            e = (l2 < 6).astype(np.float64).mean()
        else:
            sw = EC.swap_reference_free(est[None])[0]
            e = min(l2.mean(), np.sqrt(((sw - g) ** 2).sum(-1)).mean()) * 128
        out.append(e)
    return np.array(out)


def _metric_inputs(G, seed=3, N=7, K=5):
    rng = np.random.default_rng(seed)
    loc = rng.uniform(0.1, 0.9, (N, K, 2))
    W = rng.standard_normal((2 * K, 2 * G)) * 0.4
    est = ((loc.reshape(N, -1) - 0.5) @ W + 0.5).reshape(N, G, 2)
    gt = est + rng.standard_normal((N, G, 2)) * 0.02
    vis = (rng.uniform(size=(N, G)) > 0.3).astype(np.float64)
    return loc, W, gt, vis


@pytest.mark.parametrize("method", ["inter_eye_distance", "visible", "mean_average_error", "pck"])
def test_keypoint_errors_against_numpy(method):
    from stablekeypoints_amd.eval import keypoint_errors
    loc, W, gt, vis = _metric_inputs(G=6)
    vis[2] = 0                                                        # an image without a visible keypoint
    t = torch.from_numpy
    for v in (vis, None):
        got = keypoint_errors(t(loc), t(W), t(gt), None if v is None else t(v), method).numpy()
        want = _errors_numpy(loc, W, gt, v, method)
        assert got.shape == (7,) and got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)
        if method == "visible":
            assert np.isnan(got[2]) == (v is not None)
    keep = [a.copy() for a in (loc, W, gt, vis)]
    keypoint_errors(t(loc), t(W), t(gt), t(vis), method)
    assert all(np.array_equal(a, b) for a, b in zip((loc, W, gt, vis), keep))


def test_pck_threshold_hit_exactly():
    """l2 < 6 is strict: a keypoint exactly 6/256 off does not count (an identity regressor, distances representable exactly)."""
    from stablekeypoints_amd.eval import keypoint_errors
    loc = torch.full((1, 4, 2), 0.5, dtype=torch.float64)
    gt = loc.clone()
    gt[0, 0, 0] += 6 / 256                                            # exactly 6
    gt[0, 1, 1] += 6 / 256 - 2.0 ** -20                               # just inside
    gt[0, 2, 0] += 8 / 256                                            # outside
    got = keypoint_errors(loc, torch.eye(8, dtype=torch.float64), gt, None, "pck")
    assert got.tolist() == [0.5]
    assert keypoint_errors(loc, torch.eye(8, dtype=torch.float64), gt, None, "mean_average_error").item() == pytest.approx(20 - 2.0 ** -12)


def test_orientation_invariant_takes_the_nearer_of_the_two():
    from stablekeypoints_amd.eval import keypoint_errors, swap_points
    loc, W, gt, _ = _metric_inputs(G=32, seed=9, N=6)
    t = torch.from_numpy
    gt_t = t(gt)
    gt_t[1::2] = swap_points(gt_t[1::2])                              # every other image faces the other way
    got = keypoint_errors(t(loc), t(W), gt_t, None, "orientation_invariant").numpy()
    want = _errors_numpy(loc, W, gt_t.numpy(), None, "orientation_invariant")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    est = ((loc.reshape(6, -1) - 0.5) @ W + 0.5).reshape(6, 32, 2)
    plain = np.sqrt(((est - gt_t.numpy()) ** 2).sum(-1)).mean(1) * 128
    taken = got < plain - 1e-9
    assert taken.tolist() == [False, True] * 3                       # the swap branch taken and not taken
    assert np.allclose(got[~taken], plain[~taken])


def test_unknown_method_and_mismatched_shapes_raise():
    from stablekeypoints_amd.eval import keypoint_errors
    loc, W, gt, vis = (torch.from_numpy(a) for a in _metric_inputs(G=6))
    with pytest.raises(ValueError, match="evaluation method"):
        keypoint_errors(loc, W, gt, vis, "mean_error")
    with pytest.raises(ValueError, match="annotations"):
        keypoint_errors(loc, W, gt[:, :5], None, "pck")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. data and the untouched default
# ---------------------------------------------------------------------------------------------------------------------------------
def test_annotated_images_round_trip(tmp_path):
    pytest.importorskip("PIL")
    from stablekeypoints_amd import visualize as V
    from stablekeypoints_amd.custom_images import AnnotatedImages, CustomDataset
    rng = np.random.RandomState(4)
    notes, pixels = {}, {}
    for i, name in enumerate(["b.png", "a.png", "c.png"]):
        pixels[name] = rng.randint(0, 256, size=(16, 16, 3)).astype(np.uint8)
        V.write_png(str(tmp_path / name), pixels[name])
        notes[name] = {"kpts": rng.uniform(size=(4, 2)).round(4).tolist(), "visibility": [1, 0, 1, int(i > 0)]}
    (tmp_path / "annotations.json").write_text(json.dumps(notes))
    ds = AnnotatedImages(str(tmp_path), image_size=16)
    assert len(ds) == 3 and [f[-5:] for f in ds.files] == ["a.png", "b.png", "c.png"]
    plain = CustomDataset(str(tmp_path), image_size=16)
    for i, name in enumerate(["a.png", "b.png", "c.png"]):
        item = ds[i]
        assert set(item) == {"img", "kpts", "visibility"}
        assert torch.equal(item["img"], plain[i]["img"])
        assert np.array_equal((item["img"].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8), pixels[name])
        assert item["kpts"].dtype == torch.float32 and item["kpts"].tolist() == torch.tensor(notes[name]["kpts"]).tolist()
        assert item["visibility"].tolist() == [float(v) for v in notes[name]["visibility"]]
        item["kpts"].zero_()
        assert ds[i]["kpts"].abs().sum() > 0                          # items are copies
    for n in notes.values():
        del n["visibility"]
    (tmp_path / "annotations.json").write_text(json.dumps(notes))
    assert set(AnnotatedImages(str(tmp_path), 16)[0]) == {"img", "kpts"}
    del notes["c.png"]
    (tmp_path / "annotations.json").write_text(json.dumps(notes))
    with pytest.raises(KeyError):
        AnnotatedImages(str(tmp_path), 16)


def test_precompute_default_is_the_per_image_path():
    from stablekeypoints_amd import keypoint_regressor as KR
    from stablekeypoints_amd.eval import evaluate
    for f in (KR.precompute_all_keypoints, KR._precompute_all_keypoints):
        assert inspect.signature(f).parameters["batched_locator"].default is False
    names = list(inspect.signature(evaluate).parameters)
    assert names[:8] == ["ldm", "context", "indices", "regressor", "args", "controllers", "num_gpus", "from_where"]
    assert {"dataset", "routes"} <= set(names) and inspect.signature(evaluate).parameters["routes"].default == "off"


def test_fit_regressor_of_the_tool_picks_the_methods_regressor(golden):
    """tools/evaluate_keypoints.py `fit_regressor`: stage 4 of the reference's main.py on tensors -- the visible regressor with the
    visibility repeated per coordinate (ones when the dataset has none), the human3.6m loop, the plain fit; float32 out."""
    import importlib.util
    import os
    from stablekeypoints_amd import keypoint_regressor as KR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_evaluate_keypoints", os.path.join(root, "tools", "evaluate_keypoints.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, (X, Y, visible) = _case(golden, "visible")
    n = X.shape[0]
    src, tgt, vis = torch.from_numpy(X).reshape(n, -1, 2), torch.from_numpy(Y).reshape(n, -1, 2), torch.from_numpy(visible[:, ::2])
    W = tool.fit_regressor(src, tgt, vis, "visible")
    assert W.dtype == torch.float32 and torch.equal(W, torch.tensor(KR.return_regressor_visible(X, Y, visible)).float())
    torch.testing.assert_close(tool.fit_regressor(src, tgt, None, "mean_average_error"), torch.tensor(KR.return_regressor(X, Y)).float())
    assert torch.equal(tool.fit_regressor(src, tgt, vis, "pck"), torch.tensor(KR.return_regressor(X, Y)).float())
    _, (X, Y, _) = _case(golden, "h36m")
    n = X.shape[0]
    W = tool.fit_regressor(torch.from_numpy(X).reshape(n, -1, 2), torch.from_numpy(Y).reshape(n, -1, 2), None, "orientation_invariant")
    assert torch.equal(W, torch.tensor(KR.return_regressor_human36m(X, Y)).float())
