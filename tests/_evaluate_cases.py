"""Seeded inputs of the regressor tests (tests/test_evaluate_host.py) and of the tool that records the reference's answers to them
(tools/gen_eval_golden.py -> tests/golden/g14_reference_regressors.npz): built from `oracle.fixtures.seeded` by (rows, found
keypoints, annotated keypoints, seed), so the fixture holds those four numbers per case and the reference's outputs, no inputs.

    plain       a well-conditioned fit
    deficient   the last found keypoint repeats the first: X'X is singular and only the pseudo-inverse answers
    visible     per-column visibility; annotated keypoint 1 is visible in fewer rows than X has columns (pinv again)
    h36m        32 annotated joints; a third of the rows carry the left / right swapped annotation (`swap_points`), so the first
                pass of `return_regressor_human36m` swaps more than 10 rows back and the loop ends after a few passes
"""
import numpy as np
import torch

from oracle.fixtures import seeded

KINDS = ("plain", "deficient", "visible", "h36m")


def swap_reference_free(points):
    """The left / right permutation of the 32 Human3.6M joints, built here from the pair list as data (the reference's list,
    eval.py:365, including its (21, 28)): used only to PLANT swapped rows in the h36m case, never as the expected value."""
    pairs = [(1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (17, 25), (18, 26), (19, 27), (20, 28), (21, 28), (22, 30), (23, 31)]
    perm = list(range(points.shape[1]))
    for a, b in pairs:
        perm[a], perm[b] = b, a
    return points[:, perm, :]


def regressor_inputs(kind, n, k, g, seed):
    """-> (X float64 [n,2k], Y float64 [n,2g], visible float64 [n,2g] or None), locations and annotations around 0.5."""
    X = 0.5 + 0.2 * seeded((n, 2 * k), seed, torch.float64)
    if kind == "deficient":
        X[:, -2:] = X[:, :2]
    Wt = seeded((2 * k, 2 * g), seed + 1, torch.float64) * 0.6
    Y = (X - 0.5) @ Wt + 0.5 + 0.01 * seeded((n, 2 * g), seed + 2, torch.float64)
    visible = None
    if kind == "visible":
        vis = (seeded((n, g), seed + 3) > -0.5).double()
        vis[:, 1] = 0
        vis[: 2 * k - 3, 1] = 1                                     # fewer visible rows than columns of X
        visible = vis.unsqueeze(-1).repeat(1, 1, 2).reshape(n, 2 * g).numpy()
    if kind == "h36m":
        rows = torch.arange(n) % 3 == 1
        pts = Y.reshape(n, g, 2)
        pts[rows] = swap_reference_free(pts[rows])
        Y = pts.reshape(n, 2 * g)
    return X.numpy().copy(), Y.numpy().copy(), visible


def swap_input(seed):
    return seeded((2, 32, 3), seed, torch.float64)
