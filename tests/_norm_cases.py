"""Inputs, references, the error metric and the table of variants of the normalisation / pointwise edge tests
(test_norm_edges_host.py / _gpu.py): csrc/skp_group_norm.hip and csrc/skp_layer_norm.hip.

Everything here runs on the CPU with plain torch ops:

    make_gn_x / make_dy / make_ln / make_gates          one fp32 input of a family (seeded)
    check_property(kind, family, ...)                   the property that makes a family hard
    gn_case / ln_case / geglu_case                      inputs + fp64 reference + fp32 reference (kept, never modified)
    row_err(y, y64, rows)                               max_i |y_i - y64_i| / (|y64_i| + rms_row(y64)), the maximum over rows
    mean_err / rstd_err                                 |mean - mean64| * rstd64,  |rstd / rstd64 - 1|
    assert_close(got, case, form)                       err <= M[form] * max(err_fp32ref, 2^-23) + 1e-7 per output

The fp64 reference is torch's (F.group_norm / F.layer_norm / F.silu / F.gelu, autograd for the gradients).  The fp32 reference runs
the SAME ALGORITHM as the kernels in fp32 on the CPU -- mean, then the centred sum of squares, fp32 activation, fp32 autograd --
and a kernel's error is stated as a multiple of that reference's error on the same inputs.

The launch plans of csrc/skp_group_norm.hip (gn_onepass_vpt, the nsplit rule of gn_fill) and csrc/skp_layer_norm.hip (ln_plan) are
restated at the end; `assert_plan` checks every variant against the restatement AND against the library's own host queries.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

GN_FAMILIES = ("randn", "dc", "first_outlier", "last_outlier", "hot_channel", "channel_means", "constant", "saturating")
DY_FAMILIES = ("randn", "impulse", "ones")
LN_FAMILIES = ("randn", "dc", "hot_channel", "constant", "cancelling")
GATE_FAMILIES = ("randn", "tails", "far", "zero_and_tiny")
H_SCALES = (1.0, 1e4)
ABS_SLACK = 1e-7
FLOOR = 2.0 ** -23                                      # the fp32 reference's error counts as at least one ulp of 1
FLT_MIN = 2.0 ** -126
REF32_MAX = 1e-4                                        # the fp32 reference's own error stays below this: the bound hides nothing

# err_kernel <= M[form] * max(err_fp32ref, 2^-23) + ABS_SLACK: twice the largest ratio measured on the MI355X, rounded up, never
# above 8 (profiles/norm_edges.md holds the table these follow from).
M = {"gn_onepass_fwd": 8, "gn_onepass_bwd": 6, "gn_two_kernel_fwd": 3, "gn_two_kernel_bwd": 5, "gn_fork_bwd": 3, "gn_blocks_fwd": 2,
     "gn_coef": 8, "ln_fwd": 4, "ln_bwd": 5, "geglu_fwd": 2, "geglu_bwd": 4}


# ---------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------
def gn_rows(t, G):
    """[N, C, H, W] -> [N * G, L]: one row per (sample, group)."""
    return t.reshape(t.shape[0] * G, -1)


def hot_index(Cg):
    return min(1, Cg - 1)


def make_gn_x(family, shape, seed):
    assert family in GN_FAMILIES
    N, C, G, H, W = shape
    Cg = C // G
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    if family == "dc":
        x = 50 + 0.1 * x
    elif family == "first_outlier":
        gn_rows(x, G)[:, 0] = 1000.0
    elif family == "last_outlier":
        gn_rows(x, G)[:, -1] = 1000.0
    elif family == "hot_channel":
        x.view(N, G, Cg, H, W)[:, :, hot_index(Cg)] *= 100
    elif family == "channel_means":
        sign = 1.0 - 2.0 * torch.randint(0, 2, (N, C, 1, 1), generator=g)
        x = x + 20.0 * sign
    elif family == "constant":
        value = torch.where(torch.arange(N * G) % 2 == 0, 3.0, 0.0)
        x = value[:, None].expand(N * G, Cg * H * W).reshape(N, C, H, W).contiguous()
    return x


def gn_gamma_scale(family):
    return 30.0 if family == "saturating" else 1.0


def impulse_position(r, L):
    return (7 * r + 3) % L


def make_dy(family, shape, seed):
    assert family in DY_FAMILIES
    N, C, G, H, W = shape
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(N, C, H, W, generator=g)
    if family == "ones":
        dy = torch.ones_like(dy)
    elif family == "impulse":
        dy.zero_()
        rows = gn_rows(dy, G)
        for r in range(rows.shape[0]):
            rows[r, impulse_position(r, rows.shape[1])] = 1.0 + 0.25 * (r % 8)
    return dy


def make_ln(family, rows, C, seed, with_d):
    """-> (d or None, h): the row that is normalised is x = d + h."""
    assert family in LN_FAMILIES
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(rows, C, generator=g)
    d = 0.5 * torch.randn(rows, C, generator=g) if with_d else None
    if family == "dc":
        h = 50 + 0.1 * h
    elif family == "hot_channel":
        h[:, 3 % C] *= 1000
    elif family == "constant":
        value = torch.where(torch.arange(rows) % 2 == 0, 3.0, 0.0)[:, None].expand(rows, C)
        d = (value / 3.0).contiguous() if with_d else None                   # 1 + 2 and 0 + 0: exact
        h = (value - d) if with_d else value.contiguous()
    elif family == "cancelling":
        h = 4.0 * h
        d = -h + 1e-3 * torch.randn(rows, C, generator=g)                    # (always with d: the family is about the add)
    return d, h


def make_gates(family, rows, inner, seed):
    assert family in GATE_FAMILIES
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, inner, generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (rows, inner), generator=g)
    if family == "tails":                                # signs alternate: every row, even one of four gates, holds both tails (a row of
        sign = 1.0 - 2.0 * ((torch.arange(rows)[:, None] + torch.arange(inner)[None, :]) % 2)      # negative tails alone is all
        return sign * (3.0 + 3.0 * torch.rand(rows, inner, generator=g))                           # cancellation, in any fp32)
    if family == "far":
        return 40.0 * sign
    if family == "zero_and_tiny":
        table = torch.tensor([0.0, 1e-30, -1e-30, 1e-40, -1e-40])
        return table[torch.randint(0, 5, (rows, inner), generator=g)]
    return z


def check_property(kind, family, t, G=1, aux=None):
    """-> (holds, what was measured) for one input of `family`; kind: 'gn' (t = x [N,C,H,W]), 'dy', 'ln' (t = x = d + h in fp64,
    aux = (d, h)) or 'gate'."""
    td = t.double()
    if kind == "gn":
        N, C, H, W = t.shape
        Cg = C // G
        rows = gn_rows(td, G)
        L = rows.shape[1]
        if family in ("randn", "saturating"):
            m = rows.mean().abs().item()
            return m < 4 / math.sqrt(td.numel()), f"|mean| {m:.4f}"
        if family == "dc":
            ok = bool(((rows.mean(1) - 50).abs() < 0.1).all()) and bool((rows.std(1) < 0.15).all())
            return ok, f"row means {rows.mean(1).min():.2f}..{rows.mean(1).max():.2f}, std <= {rows.std(1).max():.3f}"
        if family in ("first_outlier", "last_outlier"):
            at = 0 if family == "first_outlier" else L - 1
            rest = torch.cat([rows[:, :at], rows[:, at + 1:]], 1).abs().max().item()
            return bool((rows[:, at] == 1000).all()) and rest < 10, f"element {at} of every row is 1000, the rest below {rest:.1f}"
        if family == "hot_channel":
            v = td.view(N, G, Cg, H * W).pow(2).mean(-1).sqrt()
            hot = v[:, :, hot_index(Cg)]
            others = v[:, :, [c for c in range(Cg) if c != hot_index(Cg)]]
            ok = bool((hot > 30).all()) and (Cg == 1 or bool((others < 3).all()))
            return ok, f"hot channel rms >= {hot.min():.0f}, others <= {others.max().item() if Cg > 1 else 0:.1f}"
        if family == "channel_means":
            cm = td.flatten(2).mean(-1)
            ok = bool(((cm.abs() - 20).abs() < 6 / math.sqrt(H * W) + 1e-9).all()) and bool((td.flatten(2).std(-1) < 3).all())
            return ok, f"|channel mean| {cm.abs().min():.2f}..{cm.abs().max():.2f}"
        value = torch.where(torch.arange(N * G) % 2 == 0, 3.0, 0.0).double()
        return bool((rows == value[:, None]).all()), "every row one value: 3 in the even rows, 0 in the odd ones"
    if kind == "dy":
        rows = gn_rows(td, G)
        if family == "ones":
            return bool((td == 1).all()), "all ones"
        if family == "impulse":
            nz = (rows != 0).sum(1)
            at = all(rows[r, impulse_position(r, rows.shape[1])] != 0 for r in range(rows.shape[0]))
            return bool((nz == 1).all()) and at, "one non-zero per row"
        m = td.mean().abs().item()
        return m < 4 / math.sqrt(td.numel()), f"|mean| {m:.4f}"
    if kind == "ln":
        rows, C = td.shape
        if family == "randn":
            m = td.mean().abs().item()
            return m < 4 * 1.2 / math.sqrt(td.numel()), f"|mean| {m:.4f}"
        if family == "dc":
            return bool(((td.mean(1) - 50).abs() < 1.0).all()), f"row means {td.mean(1).min():.2f}..{td.mean(1).max():.2f}"
        if family == "hot_channel":
            others = td[:, [c for c in range(C) if c != 3 % C]].abs().max().item()
            return others < 10 and td[:, 3 % C].abs().max().item() > 100, f"column {3 % C} max {td[:, 3 % C].abs().max():.0f}, others {others:.1f}"
        if family == "constant":
            value = torch.where(torch.arange(rows) % 2 == 0, 3.0, 0.0).double()
            return bool((td == value[:, None]).all()), "every row one value"
        d, h = aux
        big, small = h.abs().mean().item(), td.abs().mean().item()
        return small < 1e-3 * big, f"mean |d + h| {small:.2e} against mean |h| {big:.2f}"
    assert kind == "gate"
    a = td.abs()
    if family == "tails":
        return bool(((a >= 3) & (a <= 6)).all()) and bool((td > 0).any()) and bool((td < 0).any()), f"|g| {a.min():.2f}..{a.max():.2f}"
    if family == "far":
        return bool((a == 40).all()) and bool((td > 0).any()) and bool((td < 0).any()), "+-40"
    if family == "zero_and_tiny":
        seen = {float(v) for v in t.detach().unique()}
        return bool((a <= 1.001e-30).all()) and len(seen) >= (5 if t.numel() >= 200 else 2), f"{len(seen)} distinct values, max |g| {a.max():.3e}"
    m = td.mean().abs().item()
    return m < 4 / math.sqrt(td.numel()), f"|mean| {m:.4f}"


# ---------------------------------------------------------------------------------------------------------------------
# error metric
# ---------------------------------------------------------------------------------------------------------------------
def row_err(y, y64, rows) -> float:
    """max over rows of max_i |y_i - y64_i| / (|y64_i| + rms_row(y64) + 2^-126): an isolated huge element is judged relatively, the
    bulk against the row's typical size, a row of denormals or zeros against the smallest normal number.  NaN where y holds one (every comparison with it fails)."""
    a, b = y.double().reshape(rows, -1), y64.reshape(rows, -1)
    rms = b.pow(2).mean(1, keepdim=True).sqrt()
    e = (a - b).abs() / (b.abs() + rms + FLT_MIN)                # (below the smallest normal number fp32 has no relative precision)
    return float("nan") if bool(torch.isnan(a).any()) else e.max().item()


def mean_err(mean, mean64, rstd64) -> float:
    return ((mean.double().flatten() - mean64.flatten()).abs() * rstd64.flatten()).max().item()


def rstd_err(rstd, rstd64) -> float:
    return (rstd.double().flatten() / rstd64.flatten() - 1).abs().max().item()


def bound(e32, m) -> float:
    return m * max(e32, FLOOR) + ABS_SLACK


class Case:
    """Common part: `ref64` / `ref32` name -> tensor, `rows` name -> number of rows the metric sees, `err32` name -> the fp32
    reference's own error."""

    def finish(self):
        self.err32 = {k: self.err(k, self.ref32[k]) for k in self.ref64}

    def err(self, name, t) -> float:
        if name in ("mean", "ln_mean"):
            return mean_err(t, self.ref64[name], self.ref64["rstd" if name == "mean" else "ln_rstd"])
        if name in ("rstd", "ln_rstd"):
            return rstd_err(t, self.ref64[name])
        return row_err(t, self.ref64[name], self.rows[name])


def input_conditions(c: Case):
    """Every reference finite, no fp64 row identically zero (the metric divides by its rms), the fp32 reference's own error below
    REF32_MAX.  -> name -> that error."""
    for name, y64 in c.ref64.items():
        assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(c.ref32[name]).all()), name
        if name in c.rows and not isinstance(c, GEGLUCase):           # (a GEGLU row of zero gates IS zero, and is held to that)
            rms = y64.reshape(c.rows[name], -1).pow(2).mean(1)
            assert bool((rms > 0).all()), f"{c.what} {name}: a row of the fp64 reference is identically zero"
        assert c.err32[name] < REF32_MAX, f"{c.what} {name}: the fp32 reference is off by {c.err32[name]:.2e}"
    return c.err32


def assert_close(got, c: Case, form, m=None):
    """Every output of `got` (name -> CPU tensor) is finite and within M[form] x max(the fp32 reference's error, 2^-23) + 1e-7 of
    the fp64 reference.  One line per output; -> name -> (err, err_fp32ref).  `form`: one name, or name -> form."""
    bad, report = [], {}
    for name, t in got.items():
        f = form[name] if isinstance(form, dict) else form
        mm = m if m is not None else M[f]
        assert tuple(t.shape) == tuple(c.ref64[name].shape), f"{c.what} {name}: shape {tuple(t.shape)}"
        err, e32 = c.err(name, t), c.err32[name]
        report[name] = (err, e32)
        ratio = err / max(e32, FLOOR)
        print(f"norm-edge {c.what} {f} {name}: err {err:.3e} fp32ref {e32:.3e} ratio {ratio:.2f}")
        finite = bool(torch.isfinite(t).all())
        if not finite or not err <= bound(e32, mm):
            bad.append(f"{name}: {'NOT FINITE, ' if not finite else ''}err {err:.3e} > {mm} x max({e32:.3e}, 2^-23) + {ABS_SLACK:.0e}")
    assert not bad, f"{c.what} [{f}]: " + "; ".join(bad)
    return report


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm (+offset) (+SiLU): references
# ---------------------------------------------------------------------------------------------------------------------
def block_stats(x, nblk):
    """fp64 {mean, M2 = sum (x - mean)^2} of x [N,C,H,W] over `nblk` consecutive pixel blocks per (n, c), rounded to fp32:
    what a producing convolution's epilogue leaves behind, [N, C, nblk, 2]."""
    N, C, H, W = x.shape
    t = x.double().reshape(N, C, nblk, -1)
    mean = t.mean(-1)
    return torch.stack([mean, ((t - mean[..., None]) ** 2).sum(-1)], dim=-1).float().contiguous()


class GNCase(Case):
    def __init__(self, v, family, seed=23):
        self.v, self.family, self.what = v, family, f"{v['name']} {family}"
        N, C, G, H, W = v["shape"]
        g = torch.Generator().manual_seed(seed)
        self.gamma = (1 + 0.3 * torch.randn(C, generator=g)) * gn_gamma_scale(family)
        self.beta = 0.3 * torch.randn(C, generator=g) + 0.05
        self.off = 0.5 * torch.randn(N, C, generator=g) if v["off"] else None
        if family == "constant" and self.off is not None:
            self.off = (8 * self.off).round() / 8                 # x + off exact in fp32: with one channel per group the row stays flat,
                                                                  # and rstd = eps^-1/2 would charge the sum's rounding, 1e-3, to every fp32 norm
        self.x = make_gn_x(family, v["shape"], seed + 1)
        self.dy_family = dy_family(v, family)
        self.dy = make_dy(self.dy_family, v["shape"], seed + 2) if v["bwd"] else None
        self.dadd = torch.randn(N, C, H, W, generator=g) if v["kind"] == "fork" else None
        self.bs = block_stats(self.x, v["nblk"]) if v["nblk"] else None
        self.ref64, self.ref32 = self._reference(torch.float64), self._reference(torch.float32)
        NG = N * G
        self.rows = {"y": NG, "dx": NG, "scale": NG, "shift": NG}
        self.finish()

    def _reference(self, dtype):
        v = self.v
        N, C, G, H, W = v["shape"]
        x = self.x.to(dtype).requires_grad_(v["bwd"])
        gamma, beta = self.gamma.to(dtype), self.beta.to(dtype)
        z = x if self.off is None else x + self.off.to(dtype)[:, :, None, None]
        rows = z.reshape(N * G, -1)
        mean = rows.mean(1, keepdim=True)                         # two passes: the mean, then the centred sum of squares
        d = rows - mean
        rstd = (d * d).mean(1, keepdim=True).add(v["eps"]).rsqrt()
        out = {"mean": mean.detach().reshape(N, G), "rstd": rstd.detach().reshape(N, G)}
        if v["kind"] == "coef":
            sc = out["rstd"].repeat_interleave(C // G, 1) * gamma
            off = 0 if self.off is None else self.off.to(dtype)
            out["scale"], out["shift"] = sc, beta + (off - out["mean"].repeat_interleave(C // G, 1)) * sc
            return out
        if dtype == torch.float64:
            y = F.group_norm(z, G, gamma, beta, v["eps"])
        else:
            y = (d * rstd).reshape(N, C, H, W) * gamma[None, :, None, None] + beta[None, :, None, None]
        if v["silu"]:
            y = F.silu(y)
        out["y"] = y.detach()
        if v["bwd"]:
            (dx,) = torch.autograd.grad(y, x, self.dy.to(dtype))
            out["dx"] = dx if self.dadd is None else dx + self.dadd.to(dtype)
        return out


@functools.lru_cache(maxsize=4)
def _gn_case(name, family, seed):
    return GNCase(GN_BY_NAME[name], family, seed)


def gn_case(v, family, seed=23) -> GNCase:
    return _gn_case(v["name"], family, seed)


# ---------------------------------------------------------------------------------------------------------------------
# add + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def tree_sum(t):
    """Sum over the last dimension as a binary tree (keepdim): the order of a lane butterfly.  A running fp32 sum of 640 values
    near 50 is off by 1e-5 of their mean, which rstd = 10 turns into more than 1e-4 of the row."""
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = F.pad(t, (0, 1))
        t = t[..., 0::2] + t[..., 1::2]
    return t


class LNCase(Case):
    """x = fp32(d + h) is checked bit for bit; the norm (and its gradient) is judged on that x: ref64 = LayerNorm in fp64 of the
    fp32 sum, so the add's own rounding -- 2e-4 of a row's spread in the cancelling family -- is not charged to the norm."""

    def __init__(self, v, family, seed=31):
        self.v, self.family, self.what = v, family, f"{v['name']} {family}"
        rows, C = v["rows"], v["C"]
        g = torch.Generator().manual_seed(seed)
        self.gamma = 1 + 0.3 * torch.randn(C, generator=g)
        self.beta = 0.3 * torch.randn(C, generator=g) + 0.05
        self.with_d = v["with_d"] or family == "cancelling"
        self.d, self.h = make_ln(family, rows, C, seed + 1, self.with_d)
        self.x = self.h if self.d is None else self.d + self.h
        self.dn = torch.randn(rows, C, generator=g)
        self.dskip = torch.randn(rows, C, generator=g) if v["dskip"] else None
        self.ref64, self.ref32 = self._reference(torch.float64), self._reference(torch.float32)
        self.rows = {"n": rows, "dx": rows}
        self.finish()

    def _reference(self, dtype):
        v = self.v
        x = self.x.to(dtype).requires_grad_(True)
        gamma, beta = self.gamma.to(dtype), self.beta.to(dtype)
        mean = tree_sum(x) / v["C"]                               # the kernels' order: partial sums, then a butterfly
        d = x - mean
        rstd = (tree_sum(d * d) / v["C"]).add(v["eps"]).rsqrt()
        n = F.layer_norm(x, (v["C"],), gamma, beta, v["eps"]) if dtype == torch.float64 else d * rstd * gamma + beta
        (dx,) = torch.autograd.grad(n, x, self.dn.to(dtype))
        if self.dskip is not None:
            dx = dx + self.dskip.to(dtype)
        return {"n": n.detach(), "dx": dx, "ln_mean": mean.detach().flatten(), "ln_rstd": rstd.detach().flatten()}


@functools.lru_cache(maxsize=4)
def _ln_case(name, family, seed):
    return LNCase(LN_BY_NAME[name], family, seed)


def ln_case(v, family, seed=31) -> LNCase:
    return _ln_case(v["name"], family, seed)


# ---------------------------------------------------------------------------------------------------------------------
# GEGLU
# ---------------------------------------------------------------------------------------------------------------------
class GEGLUCase(Case):
    def __init__(self, v, gates, hscale, seed=41):
        self.v, self.family, self.what = v, gates, f"{v['name']} {gates} h*{hscale:g}"
        rows, inner = v["rows"], v["inner"]
        g = torch.Generator().manual_seed(seed)
        h = hscale * torch.randn(rows, inner, generator=g)
        self.p = torch.cat([h, make_gates(gates, rows, inner, seed + 1)], dim=1).contiguous()
        self.dy = torch.randn(rows, inner, generator=g)
        self.ref64, self.ref32 = self._reference(torch.float64), self._reference(torch.float32)
        self.rows = {"y": rows, "dh": rows, "dg": rows}
        self.finish()

    def _reference(self, dtype):
        p = self.p.to(dtype).requires_grad_(True)
        h, gate = p.chunk(2, dim=-1)
        y = h * F.gelu(gate)
        (dp,) = torch.autograd.grad(y, p, self.dy.to(dtype))
        dh, dg = dp.chunk(2, dim=-1)
        return {"y": y.detach(), "dh": dh.contiguous(), "dg": dg.contiguous()}


@functools.lru_cache(maxsize=2)
def _geglu_case(name, gates, hscale, seed):
    return GEGLUCase(GEGLU_BY_NAME[name], gates, hscale, seed)


def geglu_case(v, gates, hscale, seed=41) -> GEGLUCase:
    return _geglu_case(v["name"], gates, hscale, seed)


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated from the sources (a change there must be repeated here, and in the variants)
# ---------------------------------------------------------------------------------------------------------------------
GN_FWD_VPT, GN_BWD_VPT = (1, 2, 4, 10, 16), (1, 2, 4, 8, 10)


def gn_onepass_vpt(L, backward):
    """csrc/skp_group_norm.hip, gn_onepass_vpt: float4 per thread of the one-pass form for a row of L elements; 0: not served."""
    need = (L // 4 + 1023) // 1024
    for v in (GN_BWD_VPT if backward else GN_FWD_VPT):
        if need <= v:
            return v
    return 0


def gn_nsplit(N, G, L):
    """csrc/skp_group_norm.hip, gn_fill: workgroups per (sample, group) row of the statistics kernels."""
    rows = N * G
    want, cap = (2048 + rows - 1) // rows, max(L // 4096, 1)
    return max(1, min(want, cap, 64))


def gn_splits(L, nsplit):
    """(first float4, one past the last) of every split, as skp_gn_stats_kernel and skp_gn_finalize cut a row."""
    q4 = L // 4
    per = (q4 + nsplit - 1) // nsplit
    return [(s * per, min(s * per + per, q4)) for s in range(nsplit)]


def ln_plan(C):
    """csrc/skp_layer_norm.hip, ln_plan -> (lanes per row, float4 per lane) or None."""
    if C <= 0 or C % 4:
        return None
    for need in (2, 1):
        for lanes in (64, 32, 16, 8):
            if C % (4 * lanes):
                continue
            vv = C // (4 * lanes)
            if need <= vv <= 8 and vv != 7:
                return lanes, vv
    return None


def ln_rows_per_block(lpr):
    return 4 * (64 // lpr)


def ln_reachable():
    """(lanes per row, float4 per lane) -> the smallest width that reaches it, over every width ln_plan serves."""
    found = {}
    for C in range(4, 4 * 64 * 8 + 1, 4):
        p = ln_plan(C)
        if p is not None:
            found.setdefault(p, C)
    return found


# ---------------------------------------------------------------------------------------------------------------------
# the variants
# ---------------------------------------------------------------------------------------------------------------------
def _gn(name, kind, shape, reach, eps, off, silu, families=GN_FAMILIES, nblk=0):
    N, C, G, H, W = shape
    assert C % G == 0 and (H * W) % 4 == 0 and (not nblk or (H * W) % nblk == 0)
    return {"name": name, "kind": kind, "shape": shape, "reach": reach, "eps": eps, "off": off, "silu": silu, "families": families,
            "nblk": nblk, "bwd": kind in ("fwd_bwd", "fork"), "L": (C // G) * H * W}


ALL, BIG8, BIG64 = GN_FAMILIES, ("randn", "first_outlier", "constant"), ("randn", "first_outlier", "last_outlier", "channel_means")
GN_VARIANTS = [
    # ---- one-pass forms at their register-count boundaries; reach: float4 per thread forward / backward (0: two kernels), nsplit
    _gn("onepass-tiny-36-cg3", "fwd_bwd", (2, 96, 32, 2, 6), {"fwd": 1, "bwd": 1}, 1e-5, True, True),
    _gn("onepass-fills-1", "fwd_bwd", (1, 8, 8, 64, 64), {"fwd": 1, "bwd": 1}, 1e-6, False, False),
    _gn("onepass-first-2", "fwd_bwd", (1, 32, 32, 50, 82), {"fwd": 2, "bwd": 2}, 1e-5, True, True),
    _gn("onepass-fills-2-g1", "fwd_bwd", (2, 2, 1, 64, 64), {"fwd": 2, "bwd": 2}, 1e-6, True, False),
    _gn("onepass-first-4", "fwd_bwd", (1, 8, 8, 3, 2732), {"fwd": 4, "bwd": 4}, 1e-6, False, True),
    _gn("onepass-fills-4", "fwd_bwd", (1, 16, 4, 64, 64), {"fwd": 4, "bwd": 4}, 1e-5, True, True),
    _gn("onepass-first-10-8", "fwd_bwd", (1, 4, 4, 68, 241), {"fwd": 10, "bwd": 8}, 1e-5, False, False),
    _gn("onepass-fills-bwd-8", "fwd_bwd", (1, 8, 4, 128, 128), {"fwd": 10, "bwd": 8}, 1e-6, False, True),
    _gn("onepass-first-bwd-10", "fwd_bwd", (1, 4, 4, 12, 2731), {"fwd": 10, "bwd": 10}, 1e-6, True, False),
    _gn("onepass-fills-10", "fwd_bwd", (1, 10, 2, 64, 128), {"fwd": 10, "bwd": 10}, 1e-5, False, True),
    _gn("onepass-first-16-bwd-two-kernel", "fwd_bwd", (1, 4, 4, 28, 1463), {"fwd": 16, "bwd": 0, "nsplit": 10}, 1e-6, True, True),
    _gn("onepass-fills-16-bwd-two-kernel", "fwd_bwd", (1, 8, 2, 128, 128), {"fwd": 16, "bwd": 0, "nsplit": 16}, 1e-5, False, False),
    # ---- two kernels per direction (rows longer than 65 536 elements); q4 = 16 385 / 65 794 float4: no nsplit divides them and the
    # last split is no multiple of 256 float4
    _gn("two-kernel-nsplit-16", "fwd_bwd", (1, 32, 32, 20, 3277), {"fwd": 0, "bwd": 0, "nsplit": 16}, 1e-6, True, True),
    _gn("two-kernel-nsplit-16-plain", "fwd_bwd", (1, 8, 8, 20, 3277), {"fwd": 0, "bwd": 0, "nsplit": 16}, 1e-5, False, False),
    _gn("two-kernel-nsplit-8", "fwd_bwd", (8, 32, 32, 20, 3277), {"fwd": 0, "bwd": 0, "nsplit": 8}, 1e-6, False, True, BIG8),
    _gn("two-kernel-nsplit-64-cg2", "fwd_bwd", (1, 64, 32, 268, 491), {"fwd": 0, "bwd": 0, "nsplit": 64}, 1e-5, True, False, BIG64),
    # ---- the fork backward (dx = the norm's input gradient + the gradient of x's other use)
    _gn("fork-onepass", "fork", (1, 32, 32, 50, 82), {"fwd": 2, "bwd": 2}, 1e-6, True, True),
    _gn("fork-two-kernel", "fork", (1, 16, 8, 20, 1639), {"fwd": 0, "bwd": 0, "nsplit": 16}, 1e-5, False, False),
    # ---- statistics from a producer's block moments (synthetic: fp64 from x, rounded to fp32); Cg * nblk = 512 and 6
    _gn("blocks-fwd-nblk-64", "blocks", (1, 16, 2, 128, 128), {"fwd": 0}, 1e-6, True, True, nblk=64),
    _gn("blocks-fwd-nblk-3", "blocks", (2, 4, 2, 192, 256), {"fwd": 0}, 1e-5, False, False, nblk=3),
    # ---- the coefficient form (scale, shift per (sample, channel)); small: Cg * nblk = 8, 24, 512; own pass: skp_gn_stats_kernel
    _gn("coef-small-own-pass", "coef", (2, 16, 2, 8, 24), {"nsplit": 1}, 1e-6, True, False),
    _gn("coef-small-nblk-1", "coef", (2, 16, 2, 8, 24), {}, 1e-5, False, False, nblk=1),
    _gn("coef-small-nblk-3", "coef", (2, 16, 2, 8, 24), {}, 1e-6, True, False, nblk=3),
    _gn("coef-small-nblk-64", "coef", (2, 16, 2, 8, 24), {}, 1e-5, True, False, nblk=64),
    _gn("coef-large-own-pass", "coef", (1, 16, 2, 128, 128), {"nsplit": 32}, 1e-6, False, False),
    _gn("coef-large-own-pass-off", "coef", (1, 32, 32, 20, 3277), {"nsplit": 16}, 1e-5, True, False),
    _gn("coef-large-nblk-64", "coef", (1, 16, 2, 128, 128), {}, 1e-6, True, False, nblk=64),
]
GN_BY_NAME = {v["name"]: v for v in GN_VARIANTS}
assert len(GN_BY_NAME) == len(GN_VARIANTS)


def dy_family(v, family):
    """The dy family a (variant, x family) pair is run with: rotated so that every backward form meets every dy family.  `ones`
    is replaced where it makes the true gradient identically zero (one channel per group without SiLU: g = gamma is then constant
    along the row and dx = rstd (g - mean g - xhat mean(g xhat)) vanishes)."""
    i = (GN_VARIANTS.index(GN_BY_NAME[v["name"]]) if v["name"] in GN_BY_NAME else 0) + GN_FAMILIES.index(family)
    cand = DY_FAMILIES[i % 3]
    N, C, G, H, W = v["shape"]
    if cand == "ones" and C == G and not v["silu"]:
        cand = "randn"
    if family in ("dc", "channel_means", "constant"):
        cand = "randn"        # a large mean rounds xhat to 3e-5 in ANY fp32 arithmetic, and the structured dy amplify that: `ones` lies
    return cand               # near the null space of the backward (g - mean g cancels 16-fold), an `impulse` may sit where SiLU'
                              # crosses zero (z = -1.28) -- the fp32 reference itself is then off by 3e-4 .. 8e-4


def gn_forms(v):
    """output name -> M key, for the outputs variant `v` produces."""
    L = v["L"]
    if v["kind"] == "coef":
        return {k: "gn_coef" for k in ("mean", "rstd", "scale", "shift")}
    if v["kind"] == "blocks":
        return {k: "gn_blocks_fwd" for k in ("mean", "rstd", "y")}
    f = "gn_onepass_fwd" if gn_onepass_vpt(L, False) else "gn_two_kernel_fwd"
    b = "gn_fork_bwd" if v["kind"] == "fork" else ("gn_onepass_bwd" if gn_onepass_vpt(L, True) else "gn_two_kernel_bwd")
    return {"mean": f, "rstd": f, "y": f, "dx": b}


def _ln(name, C, rows, eps, with_d, dskip, families=LN_FAMILIES):
    return {"name": name, "C": C, "rows": rows, "eps": eps, "with_d": with_d, "dskip": dskip, "families": families, "reach": ln_plan(C)}


def _ln_variants():
    out = []
    for i, ((lpr, vv), C) in enumerate(sorted(ln_reachable().items(), key=lambda kv: kv[1])):
        out.append(_ln(f"ln-{lpr}x{vv}-w{C}", C, ln_rows_per_block(lpr) + 1, (1e-5, 1e-6)[i % 2], i % 2 == 0, i % 3 != 0))
    for i, C in enumerate((320, 640, 768, 1024, 1280)):                     # the widths of the networks
        rpb = ln_rows_per_block(ln_plan(C)[0])
        for j, rows in enumerate((1, rpb - 1, rpb + 1, 4097)):
            fams = (LN_FAMILIES[(i + j) % 5], LN_FAMILIES[(i + j + 2) % 5])
            out.append(_ln(f"ln-w{C}-rows-{rows}", C, rows, (1e-5, 1e-6)[(i + j) % 2], (i + j) % 2 == 1, j % 2 == 0, fams))
    return out


LN_VARIANTS = _ln_variants()
LN_BY_NAME = {v["name"]: v for v in LN_VARIANTS}
assert len(LN_BY_NAME) == len(LN_VARIANTS)
LN_REFUSED_WIDTH = 1792                                  # 4 * 7 * 64: seven float4 per lane is not built, and no narrower group fits

ALL_GATES = tuple((g, s) for g in GATE_FAMILIES for s in H_SCALES)
GEGLU_VARIANTS = [
    {"name": "geglu-inner-4", "rows": 259, "inner": 4, "cases": ALL_GATES},
    {"name": "geglu-inner-1280", "rows": 7, "inner": 1280, "cases": ALL_GATES},
    {"name": "geglu-inner-5120", "rows": 5, "inner": 5120, "cases": ALL_GATES},
    # rows * inner / 4 = 4 224 000 > 16 384 * 256 float4: no single trip of a full grid covers it
    {"name": "geglu-second-trip", "rows": 3300, "inner": 5120, "cases": (("tails", 1.0),)},
]
GEGLU_BY_NAME = {v["name"]: v for v in GEGLU_VARIANTS}

# (N, C, H, W) of skp_add_bias_residual_f32; the last has N*C*HW/4 = 8 421 376 float4 > 8192 blocks x 256 threads x 4: past the cap
BIAS_RESIDUAL_SHAPES = [(1, 1, 2, 2), (3, 5, 2, 6), (2, 320, 8, 8), (2, 64, 256, 260), (2, 16, 1024, 1028)]
LAYOUT_SHAPES = [(B, C, H, W) for (C, H, W) in ((4, 2, 2), (68, 12, 11), (64, 8, 8), (320, 64, 64)) for B in (1, 3)]


def assert_plan(lib, v):
    """The shape of variant `v` reaches what it is listed for, by the restated plan AND by the library's host queries."""
    if "C" in v and "shape" not in v:
        plan = ln_plan(v["C"])
        assert plan == v["reach"] and plan is not None, f"{v['name']}: plan {plan}, listed as {v['reach']}"
        assert lib.skp_add_layer_norm_ok(v["C"]) == 1
        return {"plan": plan}
    N, C, G, H, W = v["shape"]
    L = v["L"]
    facts = {"fwd": gn_onepass_vpt(L, False), "bwd": gn_onepass_vpt(L, True), "nsplit": gn_nsplit(N, G, L)}
    assert lib.skp_group_norm_onepass_ok(N, C, G, H * W) == int(facts["fwd"] > 0), "the library serves another forward form"
    assert lib.skp_group_norm_nsplit(N, C, G, H * W) == facts["nsplit"], "the library splits the rows otherwise"
    for key, want in v["reach"].items():
        assert facts[key] == want, f"{v['name']}: {key} is {facts[key]}, listed as {want}"
    if v["kind"] in ("blocks",):
        assert facts["fwd"] == 0, "a row that fits the registers never reads the block moments"
    return facts
