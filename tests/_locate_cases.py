"""Seeded cases of the keypoint locator (include/skp_locate.h; `eval.locate_keypoints`, `ops.locate`) and an independent restatement of
its definition in numpy fp64, written from the header and sharing no code with `eval.locate_formula`.

Shapes: the smallest at which each branch of the launch plan can go wrong.  `skp_locate_workspace` distinguishes
    one wave per map, four maps per workgroup      H W <= 1024          8x8, 16x16, 24x40, 5x7 (no 16-byte loads)
    one workgroup per map                          H W < 8192, or few segments wanted: 33x33 (odd), 64x64
    a map cut over several workgroups              128x128 (N = 1: 4 segments; N = 70: 4), 91x91 (odd: scalar loads, a short last
                                                   segment), 512x512 (N <= 3: 64 segments)
with N in {1, 3, 70, 300}: fewer maps than a workgroup takes, a ragged last workgroup (70 and 3 are no multiples of 4), many.

Contents, by map index modulo `len(KINDS)`: a smooth positive map (exp of a random field, as the averaged attention maps are); the
maximum in each corner and on each edge, where the window is clipped (the bottom-right corner is the very last element); exact ties
(the first must win); an all-zero map (-> (0.5, 0.5)); a constant map; all-negative values; mixed signs; one peak of 1e30 beside
values around 1e-8.

The generator rejects, in fp64,
  * a map whose two largest values are distinct and closer than one fp32 ulp (cannot happen between two float32 values; it guards a
    future change of the generator's dtype), and
  * a mixed-sign map on which some window's sum T is small beside the sum of the magnitudes (|T| < 0.25 sum |m|): the weighted
    location divides by T, so such a map measures the conditioning of the question and not the summation.

Tolerance of the weighted location.  No number is picked: tests/test_locate_host.py measures, over ALL the cases below, the largest
error in pixels of the reference-order fp32 computation (`oracle.ref_path.pixel_from_weighted_avg` on clones, on the CPU) against
the restatement, once for the windows (distance >= 0) and once for the whole-map mean (distance = -1, whose sums are long); the
kernel gets `FACTOR` = 4 times that, the project's factor for a kernel that rounds differently from torch.
"""
import functools

import numpy as np

DISTANCES = (-1, 0, 1, 2.5, 3, 5, 1000)
FACTOR = 4

# measured on the CPU (tests/test_locate_host.py::test_reference_order_fp32_error_is_what_is_recorded prints them): the largest
# error, in pixels, of oracle.ref_path.pixel_from_weighted_avg in fp32 against `restate` over all cases.  Recorded 2026-10-21.
REF_FP32_ERR_WINDOW = 4.84e-5    # distance >= 0   (n3 512x512, distance 2.5)
REF_FP32_ERR_WHOLE = 4.52e-5     # distance == -1  (n1 512x512)

#        name                N    H    W   seed
CASES = [("n1 8x8",           1,   8,   8, 11),
         ("n3 8x8",           3,   8,   8, 12),
         ("n70 8x8",         70,   8,   8, 13),
         ("n3 5x7",           3,   5,   7, 14),
         ("n70 16x16",       70,  16,  16, 15),
         ("n300 16x16",     300,  16,  16, 16),
         ("n3 24x40",         3,  24,  40, 17),
         ("n300 24x40",     300,  24,  40, 18),
         ("n1 33x33",         1,  33,  33, 19),
         ("n70 33x33",       70,  33,  33, 20),
         ("n3 64x64",         3,  64,  64, 21),
         ("n70 64x64",       70,  64,  64, 22),
         ("n300 64x64",     300,  64,  64, 23),
         ("n3 91x91",         3,  91,  91, 24),
         ("n1 128x128",       1, 128, 128, 25),
         ("n70 128x128",     70, 128, 128, 26),
         ("n1 512x512",       1, 512, 512, 27),
         ("n3 512x512",       3, 512, 512, 28)]
NAMES = [c[0] for c in CASES]

KINDS = ("smooth", "corner00", "corner0w", "cornerh0", "last", "top", "left", "bottom", "right", "ties", "zero", "constant",
         "negative", "mixed", "huge")


def _smooth(rng, H, W):
    """exp of a low-pass random field, in (0, ~20): one or two broad bumps and pixel noise."""
    ys, xs = np.mgrid[0:H, 0:W]
    f = rng.standard_normal((H, W)) * 0.3
    for _ in range(3):
        cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.3) * max(H, W)
        f += rng.uniform(0.5, 2.5) * np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * s * s))
    return np.exp(f)


def _one(kind, rng, H, W):
    m = _smooth(rng, H, W)
    top = 1.5 * m.max()
    at = {"corner00": (0, 0), "corner0w": (0, W - 1), "cornerh0": (H - 1, 0), "last": (H - 1, W - 1), "top": (0, W // 2),
          "left": (H // 2, 0), "bottom": (H - 1, W // 3), "right": (H // 3, W - 1)}
    if kind in at:
        m[at[kind]] = top
    elif kind == "ties":                                    # three equal maxima; row-major the first is (r0, c0)
        cells = rng.choice(H * W, size=min(3, H * W), replace=False)
        m.reshape(-1)[cells] = np.float32(top)
    elif kind == "zero":
        m[:] = 0.0
    elif kind == "constant":
        m[:] = 0.37
    elif kind == "negative":
        m = -m
    elif kind == "mixed":
        m = m - 0.35 * m.mean() * (1 + rng.standard_normal((H, W)))
    elif kind == "huge":
        m = m * 1e-8
        m[rng.integers(H), rng.integers(W)] = 1e30
    return m.astype(np.float32)


def _acceptable(kind, m):
    v = np.unique(m.astype(np.float64))
    if v.size > 1 and v[-1] - v[-2] < np.spacing(np.float32(v[-1])) * 0.999:
        return False
    if kind == "mixed":
        for d in DISTANCES:
            _, _, inside = _window(m[None].astype(np.float64), d)
            if abs((m * inside[0]).sum()) < 0.25 * np.abs(m * inside[0]).sum():
                return False
    return True


@functools.lru_cache(maxsize=None)
def build(name):
    """float32 [N,H,W], read-only."""
    _, N, H, W, seed = CASES[NAMES.index(name)]
    rng = np.random.default_rng(seed)
    maps = np.empty((N, H, W), dtype=np.float32)
    start = int(rng.integers(len(KINDS)))                   # a small N still meets different kinds from case to case
    for i in range(N):
        kind = KINDS[(start + i) % len(KINDS)]
        for _ in range(100):
            m = _one(kind, rng, H, W)
            if _acceptable(kind, m):
                break
        else:
            raise AssertionError(f"{name}: no acceptable {kind} map in 100 draws")
        maps[i] = m
    maps.setflags(write=False)
    return maps


def kinds(name):
    _, N, _, _, seed = CASES[NAMES.index(name)]
    start = int(np.random.default_rng(seed).integers(len(KINDS)))
    return [KINDS[(start + i) % len(KINDS)] for i in range(N)]


def _window(m, distance):
    """(flat [N], (r*, c*), inside [N,H,W] bool) of fp64 maps: the header's arg-max and window."""
    N, H, W = m.shape
    rows = m.reshape(N, -1)
    flat = (rows == rows.max(axis=1, keepdims=True)).argmax(axis=1)          # the first True
    rs, cs = flat // W, flat % W
    if distance == -1:
        return flat, (rs, cs), np.ones((N, H, W), dtype=bool)
    rr, cc = np.mgrid[0:H, 0:W]
    d2 = (rr[None] - rs[:, None, None]) ** 2 + (cc[None] - cs[:, None, None]) ** 2
    return flat, (rs, cs), np.sqrt(d2.astype(np.float32)) <= np.float32(distance)


def restate(maps, mode, distance=5):
    """The definition in fp64: float32 [N,H,W] -> (loc float64 [N,2], flat int64 [N])."""
    m = np.asarray(maps, dtype=np.float64)
    N, H, W = m.shape
    flat, (rs, cs), inside = _window(m, distance if mode == 1 else 0)
    if mode == 0:
        return np.stack([rs + 0.5, cs + 0.5], axis=1), flat
    rr, cc = np.mgrid[0:H, 0:W]
    v = np.where(inside, m, 0.0)
    T = v.sum(axis=(1, 2))
    return np.stack([(rr[None] * v).sum(axis=(1, 2)), (cc[None] * v).sum(axis=(1, 2))], axis=1) / (T + 1e-6)[:, None] + 0.5, flat


@functools.lru_cache(maxsize=None)
def want(name, mode, distance=5):
    """`restate` of a case, computed once and shared; read-only."""
    loc, flat = restate(build(name), mode, distance)
    loc.setflags(write=False)
    flat.setflags(write=False)
    return loc, flat


def tolerance(distance):
    return FACTOR * (REF_FP32_ERR_WHOLE if distance == -1 else REF_FP32_ERR_WINDOW)
