"""Cases, tolerances and an independent fp64 restatement for the overlay renderer (csrc/skp_overlay.hip, visualize.overlay_formula).

`restate` is the per-pixel definition of include/skp_overlay.h written out in numpy float64, image by image and marker by marker,
with the glyphs rasterised block by block -- it shares no code with `visualize.overlay_formula`.  It returns c * 255 BEFORE the
truncation, so the case generator can see how close a value is to a byte boundary.

The generator (`build`) is seeded per case and rejects, in fp64,
  * any point whose label box would snap within 1e-3 px of a rounding boundary (floor(centre - size / 2 + 0.5), both axes), and
  * for the cases asserted bit-exact, any byte value c * 255 within 1e-3 of an integer (the image value is nudged by 0.3 levels).

Tolerances.  Everywhere at most ONE level: the fp32 error of the blend (a few ulp of values in [0, 1], ~1e-5 levels) is orders of
magnitude below one level, so only the truncation (int)(c * 255) can move a byte, and only by one.  The share of bytes that differ at
all is capped at 4 x `FORMULA_FP32_SHARE`, the share `overlay_formula` in fp32 shows against the restatement on the same cases (the
factor is there for a kernel that rounds differently from torch, e.g. by fma contraction; the kernel as built contracts nothing);
the cases marked `exact` must be exact.
"""
import math
import struct
import zlib

import numpy as np
import torch

# measured on the CPU (tests/test_render_host.py::test_formula_fp32_within_one_level prints it): bytes of the non-exact cases on which
# overlay_formula in fp32 differs from the fp64 restatement / all their bytes.  Recorded 2026-10-20.
FORMULA_FP32_DIFFERING, FORMULA_BYTES = 1, 194994
FORMULA_FP32_SHARE = FORMULA_FP32_DIFFERING / FORMULA_BYTES
SHARE_FACTOR = 4

LUT2 = np.array([[0.1, 0.3, 0.9], [0.9, 0.7, 0.1]], dtype=np.float32)


def glyph_scale(radius, digits):
    bw = 5 if digits == 1 else 11
    return max(1, int(float(radius) / (0.5 * math.sqrt(bw * bw + 49))))


def _bilinear(mp, H, W):
    S = mp.shape[0]
    Y, X = np.mgrid[0:H, 0:W].astype(np.float64)
    sy, sx = np.maximum((Y + 0.5) * S / H - 0.5, 0.0), np.maximum((X + 0.5) * S / W - 0.5, 0.0)
    y0, x0 = np.minimum(np.floor(sy).astype(int), S - 1), np.minimum(np.floor(sx).astype(int), S - 1)
    y1, x1 = np.minimum(y0 + 1, S - 1), np.minimum(x0 + 1, S - 1)
    fy, fx = sy - y0, sx - x0
    return (1 - fy) * ((1 - fx) * mp[y0, x0] + fx * mp[y0, x1]) + fy * ((1 - fx) * mp[y1, x0] + fx * mp[y1, x1])


def restate(img, maps, pts, *, lut, colors, glyphs, alpha, radius, ring, labels):
    """fp64: img [B,3,H,W], maps [B,S,S] or None, pts [B,K,2] or None -> c * 255 as float64 [B,H,W,3] (bytes: floor)."""
    img = np.asarray(img, dtype=np.float64)
    B, _, H, W = img.shape
    alpha, radius, ring = float(np.float32(alpha)), float(np.float32(radius)), float(np.float32(ring))      # what the C entry receives
    lut = None if lut is None else np.asarray(lut, dtype=np.float64)
    out = np.empty((B, H, W, 3))
    Y, X = np.mgrid[0:H, 0:W]
    for b in range(B):
        c = np.clip(img[b].transpose(1, 2, 0), 0.0, 1.0)
        if maps is not None:
            mp = np.asarray(maps[b], dtype=np.float64)
            S, L = mp.shape[0], lut.shape[0]
            real = mp[~np.isnan(mp)]
            lo, hi = (real.min(), real.max()) if real.size else (0.0, 0.0)
            with np.errstate(all="ignore"):
                m = mp if (S == H and S == W) else _bilinear(mp, H, W)
                n = np.clip((m - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.zeros_like(m)
            n = np.where(np.isnan(m) | np.isnan(n), 0.0, n)
            t = n * (L - 1)
            i = np.minimum(t.astype(int), L - 2)
            colour = lut[i] + (t - i)[..., None] * (lut[i + 1] - lut[i])
            c = (1 - alpha) * c + alpha * colour
        K = 0 if pts is None else pts.shape[1]
        for j in range(K):
            py, px = float(pts[b, j, 0]) * H, float(pts[b, j, 1]) * W
            if math.isnan(py) or math.isnan(px):
                continue
            d = np.hypot(Y + 0.5 - py, X + 0.5 - px)
            ar = np.clip(radius + ring + 0.5 - d, 0.0, 1.0)[..., None]
            ad = np.clip(radius + 0.5 - d, 0.0, 1.0)[..., None]
            c = c + ar * (1.0 - c)
            c = c + ad * (np.asarray(colors[j], dtype=np.float64) - c)
            if labels:
                digits = [j] if j < 10 else [j // 10, j % 10]
                fs = glyph_scale(radius, len(digits))
                bw = 5 if len(digits) == 1 else 11
                oy, ox = math.floor(py - 7 * fs / 2 + 0.5), math.floor(px - bw * fs / 2 + 0.5)
                lit = np.zeros((H, W), dtype=bool)
                for k, dg in enumerate(digits):
                    for r in range(7):
                        for col in range(5):
                            if (int(glyphs[dg][r]) >> (4 - col)) & 1:
                                ya, xa = oy + r * fs, ox + (6 * k + col) * fs
                                lit[max(ya, 0):max(ya + fs, 0), max(xa, 0):max(xa + fs, 0)] = True
                c = np.where(lit[..., None], c + ad * (1.0 - c), c)
        out[b] = c * 255.0
    return out


def to_bytes(levels):
    return np.floor(levels).astype(np.int64).astype(np.uint8)


def _snap_ok(p, n, radius, two_digits):
    """The label box of a point at fraction p of n pixels snaps at least 1e-3 px away from a rounding boundary, on this axis, for the
    row extent (7 fs) and both widths (5 fs, 11 fs)."""
    c = float(np.float32(p)) * n
    sizes = {7 * glyph_scale(radius, 1), 5 * glyph_scale(radius, 1)}
    if two_digits:
        sizes |= {7 * glyph_scale(radius, 2), 11 * glyph_scale(radius, 2)}
    return all(abs((c - s / 2 + 0.5) - round(c - s / 2 + 0.5)) >= 1e-3 for s in sizes)


# name, B, H, W, S (None: no map), alpha, K, L, labels, radius, ring, flags
#   flags: exact (asserted bit-exact) | constant (hi == lo) | nanmap | edges (markers half outside each edge, two overlapping, one NaN)
#   layout (last field): None or (cols, gap, (y0, x0), pad_right, pad_bottom) -- the canvas the tiles are written into
CASES = [
    ("plain 8x8", 2, 8, 8, None, 0.7, 0, 2, True, 3.0, 1.0, {"exact"}, None),
    ("plain 16x20 vector", 2, 16, 20, None, 0.7, 0, 2, True, 3.0, 1.0, {"exact"}, None),
    ("plain 33x19 scalar", 2, 33, 19, None, 0.7, 0, 2, True, 3.0, 1.0, {"exact"}, None),
    ("plain 64x64", 1, 64, 64, None, 0.7, 0, 2, True, 3.0, 1.0, {"exact"}, None),
    ("identity map alpha 0", 2, 8, 8, 8, 0.0, 0, 2, True, 3.0, 1.0, {"exact"}, None),
    ("constant map alpha 1", 2, 8, 8, 8, 1.0, 0, 2, True, 3.0, 1.0, {"exact", "constant"}, None),
    ("identity map 64 L9", 2, 64, 64, 64, 0.7, 0, 9, True, 3.0, 1.0, set(), None),
    ("identity map with NaN", 1, 64, 64, 64, 0.7, 1, 9, True, 3.0, 1.0, {"nanmap"}, None),
    ("S 16 at 64 alpha 1", 2, 64, 64, 16, 1.0, 0, 9, True, 3.0, 1.0, set(), None),
    ("S 16 at 64 with NaN", 1, 64, 64, 16, 0.7, 0, 2, True, 3.0, 1.0, {"nanmap"}, None),
    ("S 128 at 64 K 12", 2, 64, 64, 128, 0.7, 12, 9, True, 3.0, 1.0, {"edges"}, None),
    ("S 8 at 16x20 K 1", 2, 16, 20, 8, 0.7, 1, 2, True, 4.5, 1.25, set(), None),
    ("S 12 at 33x19 K 1", 2, 33, 19, 12, 0.7, 1, 9, True, 3.0, 1.0, set(), None),
    ("markers only K 12 big", 2, 64, 64, None, 0.7, 12, 2, True, 9.0, 1.5, {"edges"}, None),
    ("markers only K 12 no labels", 1, 64, 64, None, 0.7, 12, 2, False, 5.0, 1.0, {"edges"}, None),
    ("markers K 70", 1, 64, 64, None, 0.7, 70, 2, True, 3.0, 1.0, set(), None),
    ("markers 8x8 K 1", 1, 8, 8, None, 0.7, 1, 2, True, 3.0, 1.0, set(), None),
    ("canvas 5 tiles cols 3 gap 2", 5, 16, 20, 8, 0.7, 1, 9, True, 3.0, 1.0, set(), (3, 2, (3, 5), 4, 1)),
    ("canvas vector tiles gap 4", 3, 64, 64, 64, 0.7, 2, 9, True, 5.0, 1.0, set(), (2, 4, (0, 4), 0, 2)),
    ("canvas odd origin forces scalar", 1, 16, 20, None, 0.7, 0, 2, True, 3.0, 1.0, {"exact"}, (1, 0, (1, 2), 5, 3)),
]
NAMES = [c[0] for c in CASES]
FILL = 7                                                         # what the test canvases are pre-filled with

_built = {}


def build(name):
    """The case's inputs (float32 torch tensors on the host; built once, never modified) and its restatement:
    dict(img, maps, pts, lut, colors, alpha, radius, ring, labels, layout, exact, levels [B,H,W,3] fp64, want uint8 [B,H,W,3])."""
    if name in _built:
        return _built[name]
    from stablekeypoints_amd import visualize as V
    _, B, H, W, S, alpha, K, L, labels, radius, ring, flags, layout = CASES[NAMES.index(name)]
    rs = np.random.RandomState(1000 + NAMES.index(name))
    img = rs.rand(B, 3, H, W).astype(np.float32)
    maps = None
    if S is not None:
        maps = (rs.randn(B, S, S) * 3).astype(np.float32)
        if "constant" in flags:
            maps[:] = 1.25
        if "nanmap" in flags:
            maps[:, ::5, 1::3] = np.nan
    lut = None if S is None else (LUT2 if L == 2 else V.VIRIDIS.numpy())
    pts = None
    if K:
        pts = np.empty((B, K, 2), dtype=np.float32)
        for b in range(B):
            for j in range(K):
                while True:
                    p = rs.rand(2).astype(np.float32)
                    if "edges" in flags and j < 4:               # half outside the top, bottom, left, right edge
                        p[j // 2] = np.float32((0.004, 0.996)[j % 2])
                    if "edges" in flags and j == 6:              # overlaps marker 5: drawn later, it paints over it
                        p = pts[b, 5] + np.float32(0.02) + (rs.rand(2) * 0.02).astype(np.float32)
                    if _snap_ok(p[0], H, radius, K > 10) and _snap_ok(p[1], W, radius, K > 10):
                        break
                pts[b, j] = p
        if "edges" in flags:
            pts[0, 7] = np.nan
            pts[-1, 8, 1] = np.nan
    colors = V.cycle_colors(K).numpy() if K else None
    glyphs = V.FONT_5X7.numpy()
    kw = dict(lut=lut, colors=colors, glyphs=glyphs, alpha=alpha, radius=radius, ring=ring, labels=labels)
    levels = restate(img, maps, pts, **kw)
    if "exact" in flags:
        for _ in range(4):                                       # nudge image values whose byte sits on a boundary, then look again
            near = np.abs(levels - np.round(levels)) < 1e-3
            if not near.any():
                break
            img = img + (near.transpose(0, 3, 1, 2) * np.float32(0.3 / 255)).astype(np.float32)
            levels = restate(img, maps, pts, **kw)
        assert not (np.abs(levels - np.round(levels)) < 1e-3).any(), name
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    _built[name] = dict(img=t(img), maps=t(maps), pts=t(pts), lut=t(lut), colors=t(colors), alpha=alpha, radius=radius, ring=ring,
                        labels=labels, layout=layout, exact="exact" in flags, levels=levels, want=to_bytes(levels), B=B, H=H, W=W)
    return _built[name]


def canvas_shape(case):
    """(rows, width) of the case's canvas, and the (y, x) of every tile."""
    B, H, W = case["B"], case["H"], case["W"]
    cols, gap, (y0, x0), pad_r, pad_b = case["layout"]
    at = [(y0 + (b // cols) * (H + gap), x0 + (b % cols) * (W + gap)) for b in range(B)]
    return (max(y for y, _ in at) + H + pad_b, max(x for _, x in at) + W + pad_r), at


def expected_canvas(case):
    (h, w), at = canvas_shape(case)
    canvas = np.full((h, w, 3), FILL, dtype=np.uint8)
    for b, (y, x) in enumerate(at):
        canvas[y:y + case["H"], x:x + case["W"]] = case["want"][b]
    return canvas


def compare(got, want):
    """(largest level difference, number of differing bytes, bytes)."""
    d = np.abs(np.asarray(got).astype(np.int64) - np.asarray(want).astype(np.int64))
    return int(d.max()) if d.size else 0, int((d != 0).sum()), int(d.size)


def read_png(path):
    """An 8-bit RGB PNG with filter type 0 on every row -> uint8 [H,W,3]; signature, chunk CRCs and sizes checked."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)
