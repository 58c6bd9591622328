"""Inputs, references and the error metric of the attention-map edge tests (test_map_edges_host.py / _gpu.py).

The operation under test, with logits S_l [B,H,s_l^2,NT] in log2 units as `ops.qk_logits` writes them (NT = 16*ceil(T/16), pad
columns exactly 0):

    M[b,t] = mean over (l,h) of softmax_t( bicubic_R(S_l[b,h,:,t]) )              lse[b,l*H+h] = log2 sum_t 2^bicubic_R(S_l)

bicubic = PyTorch's upsample_bicubic2d, align_corners=False, A = -0.75, tap indices clamped on access; and the gradient dS_l of
sum <M, dM> with respect to the NATURAL-log logits S_l / log2(e) (what the kernels write), for a map gradient given dense
(dM [B,T,R,R]) or as rows (sel [B,K], G [B,K,R,R]).  The `qk` variants start from q_l [B,s_l^2,C], k_l [Bk,T,C] instead and
end on dq_l, dk_l (a shared k, Bk = 1, sums over the batch).  Everything here runs on the CPU with plain torch ops:

    make_logits(family, sides, B, H, T, seed)      exact fp32 logits of one family (real columns only, pads 0)
    make_grad(v, seed)                             the map gradient of a variant: dense dM or (sel, G), randn or seam-only
    reference(...)                                 F.interpolate(bicubic) + softmax + autograd in `dtype`
    case(name, family)                             inputs + fp64 reference + fp32 reference (kept, never modified)
    check_property(family, c)                      the property that makes a family hard, on the fp64 reference
    assert_map_close(got, c, what)                 err <= M[route] * err_fp32ref + 1e-7 per output

The launch plans of the map kernels are restated at the end (a change in csrc/skp_attn_map*.hip must be repeated there);
`assert_plan` holds every variant to the plan value it is listed for.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

import _attn_cases as AT

LOG2E = 1.4426950408889634
FAMILIES = ("randn", "spike_first", "spike_last", "all_low", "all_high", "ramp", "checker", "border", "tiny")
GEOM_FAMILIES = ("randn", "checker", "border", "all_low")          # what the geometry variants run
FEW_FAMILIES = ("randn", "all_low")                                # the token counts that only complete the NT list
LONG_FAMILIES = ("randn", "spike_last", "all_low", "ramp")         # T > 128 beside the one all-family variant of a route
FAR_FAMILIES = ("randn", "spike_last", "all_low")                  # T >= 300: ten ramp blocks would push a map plane below 1e-30
QK_FAMILIES = ("randn", "spike_last", "all_low", "odd_scale", "tiny_scale")

SPIKE = 40.0            # natural-log units, as every offset below
FAR = 100.0
RAMP_STEP, RAMP_BLOCK = 8.0, 32
BORDER = 30.0
ABS_SLACK = 1e-7
PLANE_FLOOR = 1e-30     # no M64[b,t] plane maximum below this (kernel and CPU differ on denormals)
GRAD_PLANE_FLOOR = 1e-3  # no gradient plane maximum below this share of the case's largest

# err_kernel <= M[route] * err_fp32ref + ABS_SLACK: twice the largest ratio measured on the MI355X, rounded up, never above 8
# (profiles/map_edges.md holds the table the values come from).  tok and qk sit AT that cap: their largest ratios (6.6 and 6.2)
# would ask for 14 and 13, which the profile reports as findings about those cases instead of widening the bound.
M = {"fused": 3, "groups": 4, "wide": 3, "dense": 6, "dense_groups": 8, "col": 4, "tok": 8, "qk": 8}
ROUTE_KEY = {"map_fused": "fused", "map_groups": "groups", "map_wide": "wide", "map_dense": "dense",
             "map_dense_groups": "dense_groups", "map_col": "col", "map_tok": "tok"}


def nt_of(T: int) -> int:
    return (T + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def border_sites(s: int):
    """The four corners and the four edge mid-points of an s x s grid, (row, column)."""
    e, m = s - 1, s // 2
    return [(0, 0), (0, e), (e, 0), (e, e), (0, m), (e, m), (m, 0), (m, e)]


def make_logits(family, sides, B, H, T, seed=7):
    """-> [S_l [B,H,s_l^2,NT] fp32, log2 units].  Offsets are natural-log units times log2(e); columns T.. stay exactly 0."""
    assert family in FAMILIES and (family != "ramp" or T > RAMP_BLOCK)
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in sides:
        z = torch.randn(B, H, s * s, T, generator=g, dtype=torch.float64)
        if family == "randn":
            z = z * 3
        elif family in ("spike_first", "spike_last"):
            z = z * 3
            z[..., 0 if family == "spike_first" else T - 1] += SPIKE
        elif family in ("all_low", "all_high"):                  # unit spread: every logit stays beyond +-90
            z = z + (FAR if family == "all_high" else -FAR)
        elif family == "ramp":
            z = z * 3 + RAMP_STEP * (torch.arange(T) // RAMP_BLOCK).double()
        elif family == "checker":
            i = torch.arange(s)
            sign = ((-1.0) ** (i[:, None] + i[None, :])).double().reshape(s * s, 1)
            amp = 10 + 10 * torch.rand(T, generator=g, dtype=torch.float64)
            z = sign * amp + 0.1 * z
        elif family == "border":
            z = torch.zeros_like(z)
            for n, (i, j) in enumerate(border_sites(s)):        # site n on token n (mod T where T < 8)
                z[:, :, i * s + j, n % T] = BORDER
        elif family == "tiny":
            z = z * 1e-3
        S = torch.zeros(B, H, s * s, nt_of(T), dtype=torch.float32)
        S[..., :T] = (z * LOG2E).float()
        out.append(S)
    return out


def band_rows(R: int, nb: int):
    """First row of every band but the first, for `nb` bands of ceil(R / nb) rows (csrc/skp_attn_map_tok.hip)."""
    bh = (R + nb - 1) // nb
    return [m * bh for m in range(1, nb) if m * bh < R]


def make_sel(place, B, K, T, g):
    """Selected tokens [B,K] (distinct within a row): `place` puts them where the column sweep's 8-token chunks care."""
    rows = []
    for _ in range(B):
        perm = torch.randperm(T, generator=g)
        if place == "first":
            perm = torch.cat([torch.tensor([0]), perm[perm != 0]])
        elif place == "last":
            perm = torch.cat([torch.tensor([T - 1]), perm[perm != T - 1]])
        elif place == "one_chunk":                               # all of them in tokens 8..15
            assert K <= 8 and T >= 16
            perm = 8 + torch.randperm(8, generator=g)
        elif place == "none_last":                               # the last 8-token chunk holds none
            last = (T - 1) // 8 * 8
            assert K <= last
            perm = perm[perm < last]
        else:
            assert place == "random"
        rows.append(perm[:K])
    sel = torch.stack(rows)
    assert sel.shape == (B, K)
    return sel


def make_grad(v, seed=11):
    """-> (dM [B,T,R,R] or None, sel [B,K] or None, G [B,K,R,R] or None) of variant `v`."""
    g = torch.Generator().manual_seed(seed)
    B, T, R, K = v["B"], v["T"], v["R"], v["K"]
    if not v["rows"]:
        assert v["grad"] == "randn"
        return torch.randn(B, T, R, R, generator=g), None, None
    sel = make_sel(v["sel"], B, K, T, g)
    if v["grad"] == "randn":
        return None, sel, torch.randn(B, K, R, R, generator=g)
    assert v["grad"] == "seam"
    mask = torch.zeros(R, R, dtype=torch.bool)
    for i, j in border_sites(R):
        mask[i, j] = True
    for y0 in band_rows(R, v["bands"]):
        mask[y0 - 1] = mask[y0] = True
    full = mask.expand(B, K, R, R)
    n = int(full.sum())
    vals = (1 + torch.arange(n, dtype=torch.float64) / n) * (1 - 2 * (torch.arange(n) % 2)).double()     # all distinct
    G = torch.zeros(B, K, R, R)
    G[full] = vals.float()
    return None, sel, G


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def upsample(z, s, R):
    """z [B,H,s*s,T] -> [B*H,T,R,R]: the bicubic up-sampling the kernels fuse."""
    B, H, _, T = z.shape
    return F.interpolate(z.reshape(B * H, s, s, T).permute(0, 3, 1, 2), size=(R, R), mode="bicubic", align_corners=False)


def _map_of(zs, sides, H, R):
    """natural-log logits z_l [B,H,s*s,T] -> (M [B,T,R,R], lse [B,L*H,R*R] in log2 units)"""
    B, T = zs[0].shape[0], zs[0].shape[-1]
    acc, lses = 0, []
    for z, s in zip(zs, sides):
        up = upsample(z, s, R)
        lses.append((torch.logsumexp(up, dim=1) * LOG2E).reshape(B, H, R * R))
        acc = acc + up.softmax(dim=1).reshape(B, H, T, R, R).sum(dim=1)
    return acc / (len(zs) * H), torch.cat(lses, dim=1)


def _loss(Mx, dM, sel, G):
    if dM is not None:
        return (Mx * dM.to(Mx.dtype)).sum()
    return sum((Mx[b, sel[b]] * G[b].to(Mx.dtype)).sum() for b in range(Mx.shape[0]))


def reference(S, sides, H, T, R, dM, sel, G, dtype):
    """From the logits: {"M", "lse", "dS": [dL/dz_l [B,H,s*s,T]]} in `dtype`."""
    zs = [(S_l[..., :T].to(dtype) / LOG2E).requires_grad_(True) for S_l in S]
    Mx, lse = _map_of(zs, sides, H, R)
    dz = torch.autograd.grad(_loss(Mx, dM, sel, G), zs)
    return {"M": Mx.detach(), "lse": lse.detach(), "dS": [d.detach() for d in dz]}


def _heads(t, H):
    b, n, C = t.shape
    return t.reshape(b, n, H, C // H).permute(0, 2, 1, 3)


def reference_qk(qs, ks, scales, sides, H, T, R, dM, dtype):
    """From q_l, k_l: {"M", "lse", "dq": [...], "dk": [... [Bk,T,C]]} in `dtype` (autograd sums a shared k over the batch)."""
    qd = [q.detach().to(dtype, copy=True).requires_grad_(True) for q in qs]
    kd = [k.detach().to(dtype, copy=True).requires_grad_(True) for k in ks]
    zs = [(_heads(q, H) @ _heads(k, H).transpose(-1, -2)) * sc for q, k, sc in zip(qd, kd, scales)]
    Mx, lse = _map_of(zs, sides, H, R)
    grads = torch.autograd.grad(_loss(Mx, dM, None, None), qd + kd)
    L = len(qs)
    return {"M": Mx.detach(), "lse": lse.detach(), "dq": list(grads[:L]), "dk": list(grads[L:])}


# ---------------------------------------------------------------------------------------------------------------------
# error metric
# ---------------------------------------------------------------------------------------------------------------------
def plane_err(x, ref):
    """max over the leading-axis planes of max|x - ref| / max|ref[plane]|;  x, ref [P, ...].  A plane that is exactly zero (T = 1:
    the softmax of a single token has no gradient) counts with its absolute error."""
    P = ref.shape[0]
    d = (x.double() - ref.double()).reshape(P, -1).abs().amax(1)
    top = ref.double().reshape(P, -1).abs().amax(1)
    return (d / torch.where(top > 0, top, torch.ones_like(top))).max().item()


def errors(got, ref64, spike=None, scale=1.0):
    """name -> error of every output in `got`: M per (b,t) plane, lse absolute (log2 units), gradients per (b,l) plane.

    `spike` (a token index): the case puts all the mass on that token AND hands it a map gradient.  Its own logits gradient
    p_s (g_s - dot) is then pure cancellation -- 1e-12 ... 1e-8 of the terms that cancel -- and it is the largest entry of every
    plane: fp32 arithmetic (the CPU reference's softmax backward gives exactly 0 there) cannot resolve it, and the whole-plane
    metric would read 1.0 for the yardstick and let any gradient pass.  So dS is judged in two parts instead:
      "dS_rest"   the other tokens' columns, per (b,l) plane relative to their own maximum (fp32 holds these to ~1e-5);
      "dS_spike"  the spiked token's column, absolute, in units of the terms that cancel (`scale` = max|dM| / (L H)): what a
                  kernel that fails to cancel would leave behind."""
    e = {}
    for name, x in got.items():
        r = ref64[name]
        if name == "M":
            e[name] = plane_err(x.reshape(-1, *x.shape[2:]), r.reshape(-1, *r.shape[2:]))
        elif name == "lse":
            e[name] = (x.double() - r.double()).abs().max().item()
        elif name == "dS" and spike is not None:
            keep = [t for t in range(r[0].shape[-1]) if t != spike]
            e["dS_rest"] = max(plane_err(xl[..., keep], rl[..., keep]) for xl, rl in zip(x, r))
            e["dS_spike"] = max((xl[..., spike].double() - rl[..., spike]).abs().max().item() for xl, rl in zip(x, r)) / scale
        else:
            e[name] = max(plane_err(xl, rl) for xl, rl in zip(x, r))
    return e


def _finite(x):
    return all(_finite(t) for t in x) if isinstance(x, (list, tuple)) else bool(torch.isfinite(x).all())


def assert_map_close(got, c, what="", m=None):
    """Every output of `got` (CPU tensors; "dS" / "dq" / "dk" lists per layer, dS on the real columns) is finite and within
    M[route] x the fp32 reference's own error (+1e-7) of the fp64 reference: M and lse by the forward route's factor, gradients by
    the backward route's (dq / dk of the q, k variants by `qk`).  Prints one line per output; -> name -> (err,
    err_fp32ref).  `m`: one factor for all outputs instead of the routes' own."""
    v = c.v
    e = errors(got, c.ref64, c.spike, c.cancel_scale)
    bad, report = [], {}
    for name, err in e.items():
        finite = _finite(got["dS" if name.startswith("dS_") else name])
        if name == "dS_spike":                            # absolute, against the bound worked out in Case (not a multiple of the
            report[name] = (err, c.err32[name])           # reference's error: the CPU softmax backward gives an exact 0 there)
            print(f"map-edge {v['name']} {c.family} {name}: err {err:.3e} fp32ref {c.err32[name]:.3e} bound {c.spike_bound:.3e} "
                  f"share {err / c.spike_bound:.2f} [cancel]")
            if not finite or not err <= c.spike_bound:
                bad.append(f"{name}: {'NOT FINITE, ' if not finite else ''}err {err:.3e} > {c.spike_bound:.3e} of the cancelling terms")
            continue
        key = ROUTE_KEY[v["fwd"]] if name in ("M", "lse") else "qk" if v["kind"] == "qk" else ROUTE_KEY[v["bwd"]]
        mm = M[key] if m is None else m
        e32 = c.err32[name]
        report[name] = (err, e32)
        print(f"map-edge {v['name']} {c.family} {name}: err {err:.3e} fp32ref {e32:.3e} ratio "
              f"{(max(err - ABS_SLACK, 0.0) / e32 if e32 > 0 else (0.0 if err <= ABS_SLACK else math.inf)):.2f} [{key}]")
        if not finite or not err <= mm * e32 + ABS_SLACK:
            bad.append(f"{name}: {'NOT FINITE, ' if not finite else ''}err {err:.3e} > {mm} x {e32:.3e} + {ABS_SLACK:.0e}")
    assert not bad, f"{what} [{v['name']}, {c.family}]: " + "; ".join(bad)
    return report


# ---------------------------------------------------------------------------------------------------------------------
# the variants
# ---------------------------------------------------------------------------------------------------------------------
def _v(name, sides, T, R, fwd, bwd, *, H=2, B=2, K=0, rows=False, grad="randn", sel="random", wide=True, mode="dense", tune=None,
       families=GEOM_FAMILIES, reach=None, tokrow=False):
    """One launch shape.  `fwd` / `bwd`: the routes the ledger must show.  `wide`: ops.MAP_WIDE, `mode`: ops.MAP_BWD_MODE, `tune`:
    library overrides.  `rows`: the map gradient comes as K rows (`sel` places them) and not dense.  `reach`: the plan values
    the shape was chosen for (assert_plan).  `bands`: the band count the seam gradient is built for (filled in below)."""
    assert (K > 0) == rows and K <= T
    return {"name": name, "kind": "S", "sides": tuple(sides), "H": H, "T": T, "R": R, "B": B, "K": K, "fwd": fwd, "bwd": bwd,
            "rows": rows, "grad": grad, "sel": sel, "wide": wide, "mode": mode, "tune": tune or {}, "families": tuple(families),
            "reach": reach or {}, "tokrow": tokrow}


def _qk(name, sides, T, d, Bk, *, R=32, H=2, B=2):
    return {"name": name, "kind": "qk", "sides": tuple(sides), "H": H, "T": T, "R": R, "B": B, "Bk": Bk, "d": d, "K": 0,
            "fwd": "map_fused", "bwd": "map_dense", "rows": False, "grad": "randn", "sel": "random", "wide": True, "mode": "dense",
            "tune": {}, "families": QK_FAMILIES, "reach": {"gemm_scalar": bool(d % 4), "odd_k": True}, "tokrow": False}


def _families(T, fams):
    return tuple(f for f in fams if f != "ramp" or T > RAMP_BLOCK)


VARIANTS = (
    # ---- map_fused / map_dense, token axis: every NT instantiation 16 ... 128
    [_v(f"tok-axis-T{T}", (4, 8), T, 32, "map_fused", "map_dense", families=_families(T, FAMILIES), reach={"nt": [nt_of(T)]})
     for T in (1, 16, 17, 77, 100, 128)]
    + [_v(f"tok-axis-T{T}", (4, 8), T, 32, "map_fused", "map_dense", families=FEW_FAMILIES, reach={"nt": [nt_of(T)]})
       for T in (40, 60, 90)]
    # ---- map_fused / map_dense, geometry (TH rows per tile, 256-pixel segments, the quad path per layer)
    + [_v("geo-R64-s8", (8,), 20, 64, "map_fused", "map_dense", reach={"quad": (1,), "tile": ("rows", 4, False)}),
       _v("geo-R128-s16x32", (16, 32), 20, 128, "map_fused", "map_dense", reach={"quad": (1, 0), "tile": ("rows", 2, False)}),
       _v("geo-R96-s24", (24,), 20, 96, "map_fused", "map_dense", reach={"quad": (0,), "tile": ("rows", 2, False), "idle_lanes": 64}),
       _v("geo-R100-s8", (8,), 20, 100, "map_fused", "map_dense", H=1, reach={"quad": (0,), "tile": ("rows", 2, False), "idle_lanes": 56}),
       _v("geo-R10-s4", (4,), 13, 10, "map_fused", "map_dense", reach={"tile": ("rows", 25, True)}),
       _v("geo-R6-s8", (8,), 9, 6, "map_fused", "map_dense", reach={"tile": ("rows", 42, True)}),
       _v("geo-R8-s1x2", (1, 2), 16, 8, "map_fused", "map_dense", H=4, reach={"tile": ("rows", 32, True)}),
       _v("geo-R320-s16", (16,), 16, 320, "map_fused", "map_dense", H=1, B=1, reach={"quad": (0,), "tile": ("segs", 2, True)}),
       _v("geo-R512-s64", (64,), 16, 512, "map_fused", "map_dense", H=1, B=1, reach={"quad": (1,), "tile": ("segs", 2, False)})]
    # ---- token groups x two passes (MAP_WIDE off, or a shape the wide gate refuses)
    + [_v("groups-T129", (8, 16), 129, 64, "map_groups", "map_dense_groups", wide=False, families=LONG_FAMILIES, reach={"nt": [96, 48]}),
       _v("groups-T192", (8, 16), 192, 64, "map_groups", "map_dense_groups", wide=False, families=LONG_FAMILIES, reach={"nt": [96, 96]}),
       _v("groups-T200", (8, 16), 200, 64, "map_groups", "map_dense_groups", wide=False, families=FAMILIES, reach={"nt": [96, 96, 16]}),
       _v("groups-wide-refuses-R48-T130", (8, 16), 130, 48, "map_groups", "map_dense_groups", families=LONG_FAMILIES,
          reach={"nt": [96, 48], "wide_ok": False})]
    # ---- the one-pass wide forward; its backward: rows under "auto" (T > 128: the token-major sweep) or a dense gradient
    + [_v("wide-T129", (8, 16), 129, 64, "map_wide", "map_tok", K=4, rows=True, sel="last", mode="auto", families=LONG_FAMILIES, tokrow=True,
          reach={"sw": 32, "NS": 5, "auto": "sweep"}),
       _v("wide-T192", (8, 16), 192, 64, "map_wide", "map_tok", K=4, rows=True, sel="last", mode="auto", families=LONG_FAMILIES, tokrow=True,
          reach={"sw": 32, "NS": 6}),
       _v("wide-T193", (8, 16), 193, 64, "map_wide", "map_dense_groups", families=FAMILIES, tokrow=True,
          reach={"sw": 64, "NS": 4, "nt": [96, 96, 16]}),
       _v("wide-T300", (8, 16), 300, 64, "map_wide", "map_tok", K=4, rows=True, sel="last", mode="auto", families=FAR_FAMILIES, tokrow=True,
          reach={"sw": 64, "NS": 5}),
       _v("wide-T1024", (4, 8), 1024, 32, "map_wide", "map_tok", B=1, K=4, rows=True, sel="last", mode="auto", families=FAR_FAMILIES,
          tokrow=True, reach={"sw": 64, "NS": 16, "threads": 512})]
    # ---- the column sweep: 8-token chunks with / without a selected token, R / s in {4, 8}
    + [_v("col-s16-T77-K10", (16,), 77, 128, "map_fused", "map_col", K=10, rows=True, mode="col", families=FAMILIES,
          reach={"k2": (4,), "chunks": ("with", "without")}),
       _v("col-s32-T9-K1-first", (32,), 9, 128, "map_fused", "map_col", H=1, B=1, K=1, rows=True, sel="first", mode="col",
          reach={"k2": (2,), "chunks": ("with", "without")}),
       _v("col-s16-T5-K1-last", (16,), 5, 128, "map_fused", "map_col", H=5, B=1, K=1, rows=True, sel="last", mode="col",
          reach={"k2": (4,), "chunks": ("with", "without")}),
       _v("col-s16-T8-K1-first", (16,), 8, 128, "map_fused", "map_col", H=1, K=1, rows=True, sel="first", mode="col",
          reach={"k2": (4,), "chunks": ("with", "without")}),
       _v("col-mixed-T77-K8-one-chunk", (16, 16, 32), 77, 128, "map_fused", "map_col", B=1, K=8, rows=True, sel="one_chunk",
          mode="col", reach={"k2": (4, 4, 2), "chunks": ("with", "without"), "one_chunk": True}),
       _v("col-R256-s32x64-T16-K16", (32, 64), 16, 256, "map_fused", "map_col", H=1, B=1, K=16, rows=True, mode="col",
          reach={"k2": (4, 2), "chunks": ("with",)}),
       _v("col-s16-T130-K10-none-last", (16,), 130, 128, "map_wide", "map_col", H=1, K=10, rows=True, sel="none_last", mode="col",
          families=LONG_FAMILIES, reach={"k2": (4,), "chunks": ("with", "without"), "last_chunk_empty": True}),
       _v("col-s32-T200-K16", (32,), 200, 128, "map_wide", "map_col", H=1, B=1, K=16, rows=True, mode="col",
          families=LONG_FAMILIES, reach={"k2": (2,), "chunks": ("with", "without")})]
    # ---- the token-major sweep: one register class each and mixed, four heads per wave, band counts with the seam gradient
    + [_v("sweep-s8-R32-T13-K1", (8,), 13, 32, "map_fused", "map_tok", H=1, K=1, rows=True, mode="sweep",
          reach={"cls": {0}, "bands": {0: 4}}),
       _v("sweep-s16-R100-T77-K32-2bands", (16,), 77, 100, "map_fused", "map_tok", H=4, B=1, K=32, rows=True, grad="seam", mode="sweep",
          tune={"map_bands": 2}, reach={"cls": {1}, "bands": {1: 2}}),
       _v("sweep-s32-R128-T77-K32-3bands", (32,), 77, 128, "map_fused", "map_tok", H=5, B=1, K=32, rows=True, grad="seam", mode="sweep",
          tune={"map_bands": 3}, reach={"cls": {2}, "bands": {2: 3}}),
       _v("sweep-mixed-R32-T77-K4", (4, 8, 16, 32), 77, 32, "map_fused", "map_tok", H=4, K=4, rows=True, grad="seam", mode="sweep",
          families=FAMILIES, reach={"cls": {0, 1, 2}, "bands": {0: 4, 1: 4, 2: 4}}),
       _v("sweep-mixed-R32-T77-K4-1band", (4, 8, 16, 32), 77, 32, "map_fused", "map_tok", H=4, K=4, rows=True, mode="sweep",
          tune={"map_bands": 1}, reach={"cls": {0, 1, 2}, "bands": {0: 1, 1: 1, 2: 1}}),
       _v("sweep-mixed-R32-T200-K4", (4, 8, 16, 32), 200, 32, "map_wide", "map_tok", H=5, B=1, K=4, rows=True, grad="seam", mode="sweep",
          families=LONG_FAMILIES, reach={"cls": {0, 1, 2}, "bands": {0: 4, 1: 4, 2: 4}}),
       _v("sweep-mixed-R128-T13-K4", (4, 8, 16, 32), 13, 128, "map_fused", "map_tok", H=4, B=1, K=4, rows=True, grad="seam", mode="sweep",
          reach={"cls": {0, 1, 2}, "bands": {0: 16, 1: 16, 2: 16}})]
    # ---- MAP_BWD_MODE = "auto", one per branch of map_bwd_sparse_supported (the sweep at T > 128: the wide variants above)
    + [_v("auto-col", (16,), 20, 128, "map_fused", "map_col", K=4, rows=True, mode="auto", reach={"auto": "col"}),
       _v("auto-rows-scattered", (4, 8), 20, 32, "map_fused", "map_dense", K=4, rows=True, mode="auto", reach={"auto": "dense"})]
    # ---- through q, k: the fp32-MFMA GEMMs before and after the map kernels (scalar path at d % 4 != 0, odd contraction lengths)
    + [_qk("qk-d5-s5-T13-shared", (5,), 13, 5, 1),
       _qk("qk-d8-s8x16-T77-own", (8, 16), 77, 8, 2),
       _qk("qk-d40-s5-T77-own", (5,), 77, 40, 2),
       _qk("qk-d64-s8x16-T13-shared", (8, 16), 13, 64, 1),
       _qk("qk-d5-s8x16-T77-shared", (8, 16), 77, 5, 1),
       _qk("qk-d40-s8x16-T13-own", (8, 16), 13, 40, 2)]
)
BY_NAME = {v["name"]: v for v in VARIANTS}
assert len(BY_NAME) == len(VARIANTS)
CASES = [(v, f) for v in VARIANTS for f in v["families"]]


class Case:
    """Inputs of one variant on one family with the fp64 and the fp32 reference (computed once, never modified)."""

    def __init__(self, v, family, seed=7):
        self.v, self.family = v, family
        sides, H, T, R, B = v["sides"], v["H"], v["T"], v["R"], v["B"]
        self.dM, self.sel, self.G = make_grad(v)
        if v["kind"] == "qk":
            cs = [AT.make_case(family, B, v["Bk"], H, s * s, T, v["d"], seed + l) for l, s in enumerate(sides)]
            self.qs, self.ks, self.scales = [c[0] for c in cs], [c[1] for c in cs], [c[4] for c in cs]
            self.S = None
            ref = lambda dt: reference_qk(self.qs, self.ks, self.scales, sides, H, T, R, self.dM, dt)
        else:
            self.S = make_logits(family, sides, B, H, T, seed)
            ref = lambda dt: reference(self.S, sides, H, T, R, self.dM, self.sel, self.G, dt)
        # the spiked token where it holds the mass and takes a map gradient (see `errors`), the size of the terms that cancel in
        # its logits gradient, and the bound on what may be left of them: p_s = 2^(z_s - lse) is 1 up to the rounding of two
        # logits of size max|S| that the forward and the backward interpolate in different orders, so p_s (g_s - dot) keeps up to
        # a few ulp(max|S|) ln 2 of g_s / (L H); 8 ulp covers the four-tap sums on both sides.  A kernel that combines lse or dot
        # wrongly leaves 1e-2 ... 1 of them.
        self.spike, self.cancel_scale, self.spike_bound = None, 1.0, 0.0
        if v["kind"] == "S" and family in ("spike_first", "spike_last") and T > 1:
            t_s = 0 if family == "spike_first" else T - 1
            if not v["rows"] or any(t_s in row for row in self.sel.tolist()):
                g = self.dM if self.dM is not None else self.G
                self.spike, self.cancel_scale = t_s, g.abs().max().item() / (len(sides) * H)
                self.spike_bound = 8 * 2.0 ** -23 * max(S.abs().max().item() for S in self.S) * math.log(2)
        self.ref64, self.ref32 = ref(torch.float64), ref(torch.float32)
        self.err32 = errors({k: x for k, x in self.ref32.items()}, self.ref64, self.spike, self.cancel_scale)

    def logits64(self):
        """natural-log logits z_l [B,H,s*s,T] in fp64"""
        if self.S is not None:
            return [S_l[..., :self.v["T"]].double() / LOG2E for S_l in self.S]
        H = self.v["H"]
        return [(_heads(q.double(), H) @ _heads(k.double(), H).transpose(-1, -2)) * sc
                for q, k, sc in zip(self.qs, self.ks, self.scales)]


@functools.lru_cache(maxsize=6)
def _case(name, family) -> Case:
    return Case(BY_NAME[name], family)


def case(v, family) -> Case:
    return _case(v["name"], family)


# ---------------------------------------------------------------------------------------------------------------------
# what makes a family hard, measured on the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def tap_matrix(s, R, clamp=True):
    """W [R,s] fp64: one axis of the bicubic up-sampling as a matrix; `clamp` False drops the taps outside the image instead of
    folding them onto the border (the restated tap rule: src = (x + 0.5) s / R - 0.5, A = -0.75)."""
    A = -0.75
    W = torch.zeros(R, s, dtype=torch.float64)
    for x in range(R):
        src = (x + 0.5) * s / R - 0.5
        i0 = math.floor(src)
        t = src - i0
        w = [((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1, ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A]
        for j in range(4):
            i = i0 - 1 + j
            if clamp:
                W[x, min(max(i, 0), s - 1)] += w[j]
            elif 0 <= i < s:
                W[x, i] += w[j]
    return W


def check_property(family, c):
    """-> (holds, what was measured) for case `c` of `family`."""
    v = c.v
    T, R, H = v["T"], v["R"], v["H"]
    zs = c.logits64()
    M64 = c.ref64["M"]
    if v["kind"] == "qk":                                # the q, k variants: the property of _attn_cases, on these logits
        return AT.check_property(family, torch.cat(zs, dim=2), v["d"], c.scales[0])
    if family == "randn":
        m = max(z.abs().max().item() for z in zs)
        few = T * v["B"] < 8
        return 6 < m < 20 or few, f"max |logit| {m:.2f}" + (" (WAIVED: too few logits to expect 2 sigma)" if few and not 6 < m < 20 else "")
    if family in ("spike_first", "spike_last"):
        j = 0 if family == "spike_first" else T - 1
        low = M64[:, j].min().item()
        return low >= 0.999 or T == 1, f"the spiked token's map is >= {low:.6f} everywhere" + (" (T = 1: the only token, nothing to spike over)" if T == 1 else "")
    if family == "all_low":
        m = max(z.max().item() for z in zs)
        return m < -90, f"largest real logit {m:.1f}"
    if family == "all_high":
        m = min(z.min().item() for z in zs)
        return m > 90, f"smallest real logit {m:.1f}"
    if family == "ramp":
        nblk = (T + RAMP_BLOCK - 1) // RAMP_BLOCK
        mass = M64[:, (nblk - 1) * RAMP_BLOCK:].sum(1).mean().item()      # the last 32-token block holds the mass
        first = M64[:, :RAMP_BLOCK].sum(1).mean().item()
        ok = mass > 0.5 and first < math.exp(-RAMP_STEP * (nblk - 1) + 9) and nblk > 1
        return ok, f"{nblk} blocks: mean mass of the last block {mass:.3f}, of the first {first:.2e}"
    if family == "checker":
        found, ok = [], True
        for z, s in zip(zs, v["sides"]):
            over = (upsample(z, s, R).amax((2, 3)) - z.reshape(-1, s * s, T).amax(1)).min().item()     # per (b,h,t): the least
            found.append(f"s={s}: {over:+.2f}")
            if s >= 4 and R >= 2 * s:                    # a pattern to overshoot and room to do it: 0.49 x amplitude at the border
                ok = ok and over >= 3.0
            ok = ok and z.abs().max().item() >= 10
        return ok, "up-sampled maximum over low-res maximum, least over (b,h,t): " + ", ".join(found)
    if family == "border":
        found, ok = [], True
        for z, s in zip(zs, v["sides"]):
            Wc, Wz = tap_matrix(s, R), tap_matrix(s, R, clamp=False)
            img = z[0, 0].reshape(s, s, T).permute(2, 0, 1)
            up = upsample(z[:1, :1], s, R)[0]
            exact = (Wc @ img @ Wc.T - up).abs().max().item()
            diff = (Wc @ img @ Wc.T - Wz @ img @ Wz.T).abs().max().item()
            found.append(f"s={s}: clamped vs dropped taps differ by {diff:.2f} (restated taps vs interpolate {exact:.1e})")
            ok = ok and exact < 1e-11 and (diff >= 1.0 or s == R) and up.max().item() >= BORDER * 0.75
        return ok, "; ".join(found)
    if family == "tiny":
        spread = (M64.amax(1) - M64.amin(1)).max().item()
        return spread < 0.01 / T + 1e-12, f"largest (max - min over tokens) of a pixel {spread:.2e}"
    raise KeyError(family)


def input_conditions(c):
    """No plane left out of the metric: every M64[b,t] plane maximum >= 1e-30, every gradient plane maximum >= 1e-3 of the
    case's largest.  -> what was found."""
    planes = c.ref64["M"].flatten(2).amax(2)
    assert planes.min().item() >= PLANE_FLOOR, f"an M plane peaks at {planes.min().item():.1e}"
    found = {"M": planes.min().item()}
    for name in ("dS", "dq", "dk"):
        if name in c.ref64:
            mx = torch.cat([g.flatten(1).abs().amax(1) for g in c.ref64[name]])
            if c.v["T"] == 1 and name == "dS":                   # one token: the gradient is exactly zero, nothing to leave out
                assert mx.max().item() == 0
                continue
            share = (mx.min() / mx.max()).item()
            assert share >= GRAD_PLANE_FLOOR, f"a {name} plane peaks at {share:.1e} of the largest"
            found[name] = share
    return found


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated from the sources (a change there must be repeated here, and in VARIANTS)
# ---------------------------------------------------------------------------------------------------------------------
TOKEN_GROUP, GROUP_STEP = 128, 96                     # ops.py
MAX_LAYERS, XCAP = 8, 64                              # include/skp.h SKP_MAX_LAYERS, csrc/skp_attn_map.hip SKP_MAP_XCAP
COL_KMAX, COL_TC = 16, 8                              # csrc/skp_attn_map_col.hip CL_KMAX, CL_TC
TOK_KMAX, TOK_SMAX, TAP_BYTES = 32, 32, 32            # csrc/skp_attn_map_tok.hip SKP_TOK_KMAX, SKP_TOK_SMAX, sizeof(SkpTap)
E_BADARG, E_RANGE, E_LDS = -1, -2, -3


def _cdiv(a, b):
    return (a + b - 1) // b


def groups(T):
    """ops._groups"""
    return [(t0, min(T, t0 + GROUP_STEP)) for t0 in range(0, T, GROUP_STEP)]


def launch_nts(T):
    """NT instantiation of every launch of the narrow kernels (ops._map_fwd / _map_bwd, SKP_NT_SWITCH)"""
    return [nt_of(T)] if T <= TOKEN_GROUP else [nt_of(t1 - t0) for t0, t1 in groups(T)]


def fill_plan(sides, R):
    """csrc/skp_attn_map.hip fill_args / n_tiles -> {"tile": (form, TH or segs, ragged), "quad": per layer, "tiles", "idle_lanes"}"""
    if R <= 256:
        TH, TW, segs = 256 // R, R, 1
        tile, tiles, idle = ("rows", TH, R % TH != 0), _cdiv(R, TH), 256 - TH * R
    else:
        TH, TW, segs = 1, 256, _cdiv(R, 256)
        tile, tiles, idle = ("segs", segs, R % 256 != 0), R * segs, 0
    quad = tuple(int(R % s == 0 and (R // s) % 8 == 0 and R // s <= 32 and (256 % R == 0 if R <= 256 else R % 256 == 0)
                     and min(R, 256) >= XCAP) for s in sides)
    return {"tile": tile, "quad": quad, "tiles": tiles, "idle_lanes": idle, "TH": TH, "TW": TW, "segs": segs}


def dense_workspace(sides, B, H, T, R):
    """skp_attn_map_bwd_workspace (bytes); `T` = tokens of one launch"""
    segs = 1 if R <= 256 else _cdiv(R, 256)
    return 4 * B * sum(H * R * segs * s * nt_of(T) for s in sides)


def wide_plan(sides, T, R):
    """csrc/skp_attn_map_wide.hip wide_plan -> (0 or the error code, {"sw", "NS", "threads", "tiles", "lds"})"""
    if not sides or T <= 0 or R <= 0 or min(sides) <= 0:
        return E_BADARG, {}
    if len(sides) > MAX_LAYERS or T > 1024 or R > 4096 or R % 32 or max(sides) > 64:
        return E_RANGE, {}
    smax, px = max(sides), 32
    sw = 32 if T <= 192 else 64
    NS = _cdiv(T, sw)
    ncmax = min(_cdiv(px * smax, R) + 4, smax)
    p = {"sw": sw, "NS": NS, "threads": _cdiv(px * NS, 64) * 64, "tiles": R * (R // px)}
    if p["tiles"] > 65535 or p["threads"] > 512:
        return E_RANGE, p
    p["lds"] = (ncmax * (sw * NS + 4) + 2 * NS * px * 2) * 4
    return (E_LDS if p["lds"] > 160 * 1024 else 0), p


def fwd_route(sides, T, R, wide=True):
    """ops._map_fwd / ops.map_wide_supported"""
    if wide and TOKEN_GROUP < T <= 1024 and R % 32 == 0 and wide_plan(sides, T, R)[0] == 0:
        return "map_wide"
    return "map_fused" if T <= TOKEN_GROUP else "map_groups"


def col_k2(R, s):
    """csrc/skp_attn_map_col.hip col_k2: half the up-sampling ratio where the column sweep serves it, else 0"""
    if s < 8 or R % s:
        return 0
    return R // s // 2 if R // s in (4, 8) else 0


def col_ok(sides, H, T, R, K):
    """skp_attn_map_bwd_col_ok"""
    return int(0 < len(sides) <= MAX_LAYERS and H > 0 and 0 < T <= 1024 and 0 < K <= COL_KMAX and R in (128, 256)
               and all(col_k2(R, s) and s <= 64 and s % 4 == 0 for s in sides))


def col_workspace(sides, B, H, T, R, K):
    """skp_attn_map_bwd_col_workspace (bytes)"""
    if not col_ok(sides, H, T, R, K):
        return E_RANGE
    return 4 * (2 * B * len(sides) * H * R * R + sum(B * H * s * s * COL_KMAX for s in sides)) + 64


def col_chunks(sel, T):
    """Which kinds of 8-token chunk the sweep meets: with / without a selected token (per batch row, over all rows)."""
    kinds = set()
    for row in sel.tolist():
        hit = {t // COL_TC for t in row}
        kinds |= {"with" if ch in hit else "without" for ch in range(nt_of(T) // COL_TC)}
    return tuple(sorted(kinds))


def tok_class(s):
    """skp_tok_class: the register class of a layer side (<= 8 | <= 16 | <= 32)"""
    return 0 if s <= 8 else 1 if s <= 16 else 2


def tok_bands(sides, cls, B, H, T, R, forced=0):
    """skp_tok_bands: bands of the launch of register class `cls`; `forced` = the map_bands override"""
    if forced:
        return min(forced, R)
    cols = sum(tok_class(s) == cls for s in sides) * B * _cdiv(H, 4) * _cdiv(T, 16)
    nb = 1
    while cols * nb < 6144 and R // (nb * 2) >= 8:
        nb *= 2
    return nb


def tok_cap(R, s, bh):
    return _cdiv(bh * s, R) + 4


def sparse_workspace(sides, B, H, T, R, K, forced=0):
    """skp_attn_map_bwd_sparse_workspace (bytes): tap tables, (lse, dot) pairs, band partials where a class runs > 1 band"""
    if K > TOK_KMAX or R > 1024 or max(sides) > TOK_SMAX:
        return E_RANGE
    tab = (R * TAP_BYTES + 128 + (TOK_SMAX + 4) * 4 + 31) // 32 * 32
    n = len(sides) * tab + B * len(sides) * H * R * R * 8
    for s in sides:
        nb = tok_bands(sides, tok_class(s), B, H, T, R, forced)
        if nb > 1:
            n += B * H * nb * tok_cap(R, s, _cdiv(R, nb)) * s * nt_of(T) * 4
    return n + 64


def bwd_route(v):
    """ops._stack_grads / map_bwd_sparse_supported / _map_bwd_sparse for variant `v`"""
    sides, H, T, R, K, mode = v["sides"], v["H"], v["T"], v["R"], v["K"], v["mode"]
    dense = "map_dense" if T <= TOKEN_GROUP else "map_dense_groups"
    if not v["rows"] or mode == "dense":
        return dense
    col = mode != "sweep" and T <= 1024 and col_ok(sides, H, T, R, K)
    sweep = mode != "col" and max(sides) <= 32 and 1 <= K <= 32 and R <= 1024
    sparse = col or (sweep and T > TOKEN_GROUP) if mode == "auto" else col or sweep
    if not sparse:
        return dense
    return "map_col" if col else "map_tok"


def variant_bands(v):
    """cls -> band count of the token-major sweep for variant `v`"""
    forced = v["tune"].get("map_bands", 0)
    return {cls: tok_bands(v["sides"], cls, v["B"], v["H"], v["T"], v["R"], forced) for cls in {tok_class(s) for s in v["sides"]}}


for _x in VARIANTS:                                   # the band count the seam gradient of a sweep variant is built around
    _x["bands"] = max(variant_bands(_x).values()) if _x["bwd"] == "map_tok" else 1


def plan_facts(v, sel=None):
    """Every plan value of variant `v` by the restatement."""
    sides, H, T, R, B, K = v["sides"], v["H"], v["T"], v["R"], v["B"], v["K"]
    f = dict(fill_plan(sides, R), nt=launch_nts(T), fwd=fwd_route(sides, T, R, v["wide"]), bwd=bwd_route(v))
    f["wide_ok"] = wide_plan(sides, T, R)[0] == 0
    if f["fwd"] == "map_wide":
        f.update({k: x for k, x in wide_plan(sides, T, R)[1].items() if k != "tiles"})
    if f["bwd"] == "map_col":
        f["k2"] = tuple(col_k2(R, s) for s in sides)
        if sel is not None:
            f["chunks"] = col_chunks(sel, T)
            f["one_chunk"] = all(len({t // COL_TC for t in row}) == 1 for row in sel.tolist())
            f["last_chunk_empty"] = all(max(row) // COL_TC < (T - 1) // COL_TC for row in sel.tolist())
    if f["bwd"] == "map_tok":
        f["cls"], f["bands"] = {tok_class(s) for s in sides}, variant_bands(v)
    if v["rows"] and v["mode"] == "auto":
        f["auto"] = {"map_col": "col", "map_tok": "sweep"}.get(f["bwd"], "dense")
    if v["kind"] == "qk":
        f["gemm_scalar"] = bool(v["d"] % 4)
        f["odd_k"] = bool(T % 2) or any((s * s) % 2 for s in sides)
    return f


def assert_plan(ops, v):
    """Variant `v` reaches the routes and the plan values it is listed for: the restatement against `v["reach"]`, and against the
    library's host queries (call it with the variant's overrides set).  -> the facts."""
    lib, N = ops.N.lib(), ops.N
    sides, H, T, R, B, K = v["sides"], v["H"], v["T"], v["R"], v["B"], v["K"]
    sel = make_grad(v)[1]
    f = plan_facts(v, sel)
    assert f["fwd"] == v["fwd"] and f["bwd"] == v["bwd"], (f["fwd"], f["bwd"])
    for key, want in v["reach"].items():
        assert f.get(key) == want, f"{v['name']}: {key} is {f.get(key)!r}, listed for {want!r}"
    si, _keep = N.int_array(sides)
    assert bool(lib.skp_attn_map_fwd_wide_ok(si, len(sides), T, R)) == f["wide_ok"]
    if v["bwd"] in ("map_dense", "map_dense_groups"):
        Tl = T if T <= TOKEN_GROUP else GROUP_STEP
        assert lib.skp_attn_map_bwd_workspace(si, len(sides), B, H, Tl, R) == dense_workspace(sides, B, H, Tl, R)
    if v["rows"]:
        assert lib.skp_attn_map_bwd_col_ok(si, len(sides), H, T, R, K) == col_ok(sides, H, T, R, K)
        assert (v["bwd"] == "map_col") == bool(col_ok(sides, H, T, R, K) and v["mode"] != "sweep")
    if v["bwd"] == "map_col":
        assert lib.skp_attn_map_bwd_col_workspace(si, len(sides), B, H, T, R, K) == col_workspace(sides, B, H, T, R, K)
    if v["bwd"] == "map_tok":
        forced = v["tune"].get("map_bands", 0)
        assert lib.skp_tune_get(b"map_bands") == forced
        assert lib.skp_attn_map_bwd_sparse_workspace(si, len(sides), B, H, T, R, K) == sparse_workspace(sides, B, H, T, R, K, forced), \
            "the library plans another band count for this shape"
    return f
