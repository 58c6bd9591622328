#!/usr/bin/env python
"""Writes tests/golden/g14_reference_regressors.npz: the REFERENCE's own `return_regressor`, `return_regressor_visible`,
`return_regressor_human36m` (keypoint_regressor.py:201-273) and `swap_points` (eval.py:360-371) on the seeded inputs of
tests/_evaluate_cases.py.  Needs the reference checkout that `oracle.gen_golden.import_reference()` imports; no test imports this
file.  The fixture holds DATA only: (rows, found keypoints, annotated keypoints, seed) per case and the reference's outputs, plus
the number of passes its human3.6m loop took.

    python tools/gen_eval_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

#        kind          rows  found  annotated  seed
CASES = {"plain":     (120,     5,         4,  1401),
         "deficient": (90,      5,         3,  1411),
         "visible":   (60,      5,         4,  1421),
         "h36m":      (210,     4,        32,  1431)}
SWAP_SEED = 1441


def main():
    import _evaluate_cases as EC
    from oracle.gen_golden import import_reference
    _, _, _, ref_eval, _ = import_reference()
    from unsupervised_keypoints import keypoint_regressor as ref_kr

    out = {"swap/seed": np.array(SWAP_SEED), "swap/out": ref_eval.swap_points(EC.swap_input(SWAP_SEED)).numpy()}
    for kind, (n, k, g, seed) in CASES.items():
        X, Y, visible = EC.regressor_inputs(kind, n, k, g, seed)
        keep = Y.copy()
        out[kind + "/spec"] = np.array([n, k, g, seed])
        if kind == "visible":
            W = ref_kr.return_regressor_visible(X, Y, visible)
        elif kind == "h36m":
            passes, real = [0], ref_eval.swap_points

            def counting(points):
                passes[0] += 1
                return real(points)
            ref_eval.swap_points = counting
            try:
                W = ref_kr.return_regressor_human36m(X, Y)
            finally:
                ref_eval.swap_points = real
            out["h36m/passes"] = np.array(passes[0])
            assert 2 <= passes[0] < 10, passes
        else:
            W = ref_kr.return_regressor(X, Y)
        assert np.array_equal(Y, keep)
        out[kind + "/W"] = np.asarray(W, dtype=np.float64)
        print(kind, out[kind + "/W"].shape, "rank of X'X:", np.linalg.matrix_rank((X - 0.5).T @ (X - 0.5)), "of", 2 * k)
    path = os.path.join(ROOT, "tests", "golden", "g14_reference_regressors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; human3.6m passes:", int(out["h36m/passes"]))


if __name__ == "__main__":
    main()
