"""Inputs, references and the error metric of the attention-edge tests (test_attention_edges_host.py / _gpu.py).

The core under test is  out = softmax(scale q k^T) v  per head, q [B,N,H*d], k / v [Bk,Nk,H*d] with Bk in {1, B}, and its
gradients for a given dout.  Everything here runs on the CPU with plain torch ops:

    make_case(family, B, Bk, H, N, Nk, d, seed) -> q, k, v, dout, scale      exact fp32 inputs of one input family
    reference(q, k, v, dout, scale, H, dtype)                                materialised reference in `dtype`
    case(family, B, Bk, H, N, Nk, d)                                         inputs + fp64 reference + fp32 reference (kept)
    check_property(family, logits, d, scale)                                 the property that makes a family hard
    assert_attn_close(got, case, m, what)                                    err <= m * err_fp32ref + 1e-7 per output

The families control the LOGITS, not only the inputs.  Every head has a unit vector u_h; the random parts of q and k are made
orthogonal to it, then a u_h goes onto every query and c_j u_h onto key j, so that
    logit[i][j] = scale q_perp[i].k_perp[j]  +  scale a c_j
with the second term an offset chosen per key (the cross terms vanish up to fp32 rounding of the inputs).  `scale` is always a
value fp32 holds exactly, so the fp64 reference and a kernel that takes a float see the same number.

The softmax here runs over keys; the attention-MAP kernels normalise over tokens instead, and can reuse the families by swapping
the roles of q and k.
"""
from __future__ import annotations

import functools
import math

import torch

FAMILIES = ("randn", "spike_first", "spike_mid", "spike_last", "ramp_up", "ramp_down", "all_high", "all_low", "onehot",
            "odd_scale", "tiny_scale")
# the families a long-sequence variant (N >= 1024) runs
LONG_FAMILIES = ("randn", "spike_last", "ramp_up", "all_high", "all_low", "odd_scale")

SPIKE = 12.0          # factor on the spiked key row (x8 tops out at logits of 17-20 on the few hundred rows of the smallest shapes)
BLOCK = 32            # key block of the ramp families' property (the smallest key tile of any kernel here)
RAMP_STEP = 8.0       # logit offset added per key block
FAR = 100.0           # |offset| of all_high / all_low
ABS_SLACK = 1e-7

# err_kernel <= M[kernel family] * err_fp32ref + ABS_SLACK: twice the largest ratio measured on the MI355X, rounded up, and never
# above 8 (profiles/attention_edges.md).  flash_f32 and gen1 sit AT that cap: their largest ratios (7.4 and 4.6) would ask for
# 15 and 10, which the table there reports as findings about those kernels instead of widening the bound.
M = {"flash_f32": 8, "flash_split": 5, "cross": 7, "gen1": 8}


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _heads(t, H):
    b, n, C = t.shape
    return t.reshape(b, n, H, C // H)


def _along(t, u, H):
    """Remove the u_h component of every head's slice of t (fp64)."""
    th = _heads(t, H)
    return (th - (th * u).sum(-1, keepdim=True) * u).reshape(t.shape)


def make_case(family, B, Bk, H, N, Nk, d, seed=7):
    """-> q [B,N,C], k, v [Bk,Nk,C], dout [B,N,C] (fp32), scale (a float that fp32 holds exactly)."""
    assert family in FAMILIES and Bk in (1, B)
    g = torch.Generator().manual_seed(seed)
    C = H * d
    q = torch.randn(B, N, C, generator=g)
    k = torch.randn(Bk, Nk, C, generator=g)
    v = torch.randn(Bk, Nk, C, generator=g)
    dout = torch.randn(B, N, C, generator=g)
    u = torch.randn(H, d, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    scale = _f32(d ** -0.5)
    if family == "odd_scale":
        scale = _f32(0.37)
    elif family == "tiny_scale":
        scale = _f32(1e-3)
    elif family.startswith("spike_"):
        k[:, {"spike_first": 0, "spike_mid": Nk // 2, "spike_last": Nk - 1}[family]] *= SPIKE
    elif family == "onehot":
        q, k = q * 6.0, k * 6.0
    elif family in ("ramp_up", "ramp_down", "all_high", "all_low"):
        blk = torch.arange(Nk, dtype=torch.float64) // BLOCK
        off = {"ramp_up": RAMP_STEP * blk, "ramp_down": RAMP_STEP * (blk[-1] - blk),
               "all_high": torch.full((Nk,), FAR, dtype=torch.float64),
               "all_low": torch.full((Nk,), -FAR, dtype=torch.float64)}[family]
        top = off.abs().max().item()
        if top > 0:                                   # (a ramp over a single key block is flat: nothing to add)
            a = math.sqrt(top / scale)                # the offset split evenly between q and k
            c = off / (a * scale)
            q = (_heads(_along(q.double(), u, H), H) + a * u).reshape(B, N, C).float()
            k = (_heads(_along(k.double(), u, H), H) + c[None, :, None, None] * u).reshape(Bk, Nk, C).float()
    return q, k, v, dout, scale


def _split(t, H, dtype):
    b, n, C = t.shape
    return t.to(dtype).reshape(b, n, H, C // H).permute(0, 2, 1, 3)


def _merge(t):
    b, H, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, H * d)


def logits(q, k, scale, H, dtype=torch.float64):
    """[B,H,N,Nk] scale q k^T, materialised."""
    return (_split(q, H, dtype) @ _split(k, H, dtype).transpose(-1, -2)) * scale


def backward_from(P, out_h, qh, kh, vh, gh, scale):
    """(dq, dk rows, dv rows), heads merged, from the probabilities P [B,H,N,Nk] and the per-head out; dk / dv hold one
    [Nk,C] gradient PER BATCH ROW (what the C ABI writes for a shared k / v)."""
    dP = gh @ vh.transpose(-1, -2)
    D = (gh * out_h).sum(-1, keepdim=True)
    dS = P * (dP - D)
    return _merge((dS @ kh) * scale), _merge((dS.transpose(-1, -2) @ qh) * scale), _merge(P.transpose(-1, -2) @ gh)


def reference(q, k, v, dout, scale, H, dtype):
    """Materialised softmax attention and its gradients in `dtype`: out [B,N,C], lse [B,H,N] (natural log), dq [B,N,C],
    dk / dv [B,Nk,C] per batch row."""
    qh, kh, vh, gh = (_split(t, H, dtype) for t in (q, k, v, dout))
    S = (qh @ kh.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    out_h = P @ vh
    dq, dk, dv = backward_from(P, out_h, qh, kh, vh, gh, scale)
    return {"out": _merge(out_h), "lse": lse, "dq": dq, "dk": dk, "dv": dv}


class Case:
    """Inputs of one family at one shape with the fp64 and the fp32 reference (computed once, never modified)."""

    def __init__(self, family, B, Bk, H, N, Nk, d, seed=7):
        self.family, self.shape = family, (B, Bk, H, N, Nk, d)
        self.q, self.k, self.v, self.dout, self.scale = make_case(family, B, Bk, H, N, Nk, d, seed)
        self.H = H
        self.shared = Bk == 1 and B > 1
        self.ref64 = reference(self.q, self.k, self.v, self.dout, self.scale, H, torch.float64)
        self.ref32 = reference(self.q, self.k, self.v, self.dout, self.scale, H, torch.float32)
        self.err32 = errors(self.ref32, self.ref64, self.shared)

    def logits(self):
        return logits(self.q, self.k, self.scale, self.H)


@functools.lru_cache(maxsize=24)
def case(family, B, Bk, H, N, Nk, d, seed=7) -> Case:
    return Case(family, B, Bk, H, N, Nk, d, seed)


# ---------------------------------------------------------------------------------------------------------------------
# error metric
# ---------------------------------------------------------------------------------------------------------------------
def rel_err(x, x64) -> float:
    """max |x - x64| / max |x64|"""
    return ((x.double() - x64).abs().max() / x64.abs().max()).item()


def rows_err(x, x64) -> float:
    """The worst batch row of rel_err: every row of a [B,Nk,C] gradient against its own sample's maximum."""
    return max(rel_err(x[b], x64[b]) for b in range(x64.shape[0]))


def errors(got, ref64, shared):
    """name -> error of every output `got` holds: out / dq relative to the maximum, lse absolute, dk / dv per batch row;
    `shared` (one k / v for B > 1 rows) adds the summed gradients dk_sum / dv_sum, added up as the caller would."""
    e = {}
    for name, x in got.items():
        if name == "lse":
            e[name] = (x.double() - ref64[name]).abs().max().item()
        elif name in ("dk", "dv"):
            e[name] = rows_err(x, ref64[name])
            if shared:
                e[name + "_sum"] = rel_err(x.sum(dim=0), ref64[name].sum(dim=0))
        else:
            e[name] = rel_err(x, ref64[name])
    return e


def assert_attn_close(got, c: Case, m, what=""):
    """Every output of `got` (name -> CPU tensor, dk / dv as [B,Nk,C] rows) is finite and within m x the fp32 materialised
    reference's own error (+1e-7) of the fp64 reference.  Prints one line per output; -> name -> (err, err_fp32ref)."""
    for name, x in got.items():
        assert tuple(x.shape) == tuple(c.ref64[name].shape), f"{what} {name}: shape {tuple(x.shape)}"
    e = errors(got, c.ref64, c.shared)
    bad, report = [], {}
    for name, err in e.items():
        e32 = c.err32[name]
        need = max(err - ABS_SLACK, 0.0) / e32 if e32 > 0 else (0.0 if err <= ABS_SLACK else math.inf)
        report[name] = (err, e32)
        print(f"attn-edge {what} {c.family} {name}: err {err:.3e} fp32ref {e32:.3e} ratio {err / e32 if e32 > 0 else math.inf:.2f} "
              f"needs_m {need:.2f}")
        finite = bool(torch.isfinite(got[name.replace("_sum", "")]).all())
        if not finite or not err <= m * e32 + ABS_SLACK:
            bad.append(f"{name}: {'NOT FINITE, ' if not finite else ''}err {err:.3e} > {m} x {e32:.3e} + {ABS_SLACK:.0e}")
    assert not bad, f"{what} [{c.family}, (B,Bk,H,N,Nk,d)={c.shape}]: " + "; ".join(bad)
    return report


# ---------------------------------------------------------------------------------------------------------------------
# what makes a family hard: conditions on the fp64 logits
# ---------------------------------------------------------------------------------------------------------------------
def _block_max(S):
    """[..., nblocks]: maximum of every BLOCK-key block (the last one may be ragged)."""
    return torch.stack([S[..., j:j + BLOCK].amax(-1) for j in range(0, S.shape[-1], BLOCK)], dim=-1)


def check_property(family, S, d, scale):
    """-> (holds, what was measured) for the fp64 logits S [B,H,N,Nk] of `family`."""
    Nk = S.shape[-1]
    P = torch.softmax(S, dim=-1)
    if family == "randn":
        m = S.abs().max().item()
        return m < 8, f"max |logit| {m:.2f}"
    if family.startswith("spike_"):
        j = {"spike_first": 0, "spike_mid": Nk // 2, "spike_last": Nk - 1}[family]
        top, frac = S.max().item(), (S.argmax(-1) == j).double().mean().item()
        return top >= 20 and frac >= 0.25, f"max logit {top:.1f}, key {j} is the row maximum in {frac:.2f} of the rows"
    if family in ("ramp_up", "ramp_down"):
        bm = _block_max(S)
        step = bm[..., 1:] - bm[..., :-1] if family == "ramp_up" else bm[..., :-1] - bm[..., 1:]
        frac = (step >= 2).all(-1).double().mean().item()
        return frac >= 0.9, f"every block maximum moves by >= 2 in {frac:.3f} of the rows ({bm.shape[-1]} blocks)"
    if family == "all_high":
        return S.min().item() >= 90, f"min logit {S.min().item():.1f}"
    if family == "all_low":
        return S.max().item() <= -90, f"max logit {S.max().item():.1f}"
    if family == "onehot":
        m = P.amax(-1).mean().item()
        return m >= 0.9, f"mean of the largest weight per row {m:.3f}"
    if family == "odd_scale":
        return abs(scale - d ** -0.5) > 1e-2 * d ** -0.5, f"scale {scale} vs {d ** -0.5:.4f}"
    if family == "tiny_scale":
        spread = (P.amax(-1) - P.amin(-1)).max().item()
        return spread < 0.01, f"largest (max P - min P) of a row {spread:.2e}"
    raise KeyError(family)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel variants and the smallest shape that reaches each (gates: csrc/skp_flash_attn.hip skp_fa2_fwd / skp_fa2_bwd /
# fa2_two_kernel_splits / fa2_fused_ok / fa2_fused_splits, csrc/skp_flash_attn_s.hip skp_flash_attn_fwd_split_f32,
# csrc/skp_cross_attn.hip ca_use_ts; restated beside the GPU tests, which assert that each shape lands where this table says)
# ---------------------------------------------------------------------------------------------------------------------
def _v(name, kernel, B, Bk, H, N, Nk, d, fwd, bwd=None, tune=None, families=FAMILIES):
    return {"name": name, "kernel": kernel, "shape": (B, Bk, H, N, Nk, d), "fwd": fwd, "bwd": bwd, "tune": tune or {},
            "families": families}


VARIANTS = [
    # ---- flash, fp32 instructions.  fwd: "q128" / "q256" = 32 / 64 queries per wave, "d160" / "d160_halves";
    #      bwd: ("two_kernel", range splits) / ("fused", key-range splits)
    _v("f32-d40-shared", "flash_f32", 2, 1, 2, 130, 200, 40, "q128", ("two_kernel", 1)),
    _v("f32-d40-own", "flash_f32", 2, 2, 2, 130, 200, 40, "q128", ("two_kernel", 1)),
    _v("f32-d40-biggrid", "flash_f32", 64, 1, 8, 70, 130, 40, "q256", ("two_kernel", 1)),
    _v("f32-d64-shared", "flash_f32", 2, 1, 2, 130, 200, 64, "q128", ("two_kernel", 1)),
    _v("f32-d64-own", "flash_f32", 2, 2, 2, 130, 200, 64, "q128", ("two_kernel", 1)),
    _v("f32-d80-shared", "flash_f32", 2, 1, 2, 130, 200, 80, "q128", ("two_kernel", 1)),
    _v("f32-d80-own", "flash_f32", 2, 2, 2, 130, 200, 80, "q128", ("two_kernel", 1)),
    _v("f32-d160-plain-1split", "flash_f32", 2, 1, 2, 100, 100, 160, "d160", ("two_kernel", 1)),
    _v("f32-d160-halves-2split-shared", "flash_f32", 2, 1, 2, 130, 200, 160, "d160_halves", ("two_kernel", 2)),
    _v("f32-d160-halves-2split", "flash_f32", 1, 1, 2, 200, 160, 160, "d160_halves", ("two_kernel", 2)),
    _v("f32-d160-halves-4split", "flash_f32", 1, 1, 2, 288, 288, 160, "d160_halves", ("two_kernel", 4)),
    _v("f32-d40-fused", "flash_f32", 1, 1, 2, 1100, 1100, 40, "q128", ("fused", 1), families=LONG_FAMILIES),
    _v("f32-d64-fused", "flash_f32", 1, 1, 2, 1100, 1100, 64, "q128", ("fused", 1), families=LONG_FAMILIES),
    _v("f32-d80-fused-keysplit", "flash_f32", 1, 1, 2, 1100, 1100, 80, "q128", ("fused", 2), families=LONG_FAMILIES),
    _v("f32-d80-fused-sd15-32sq", "flash_f32", 1, 1, 18, 1024, 1024, 80, "q128", ("fused", 1), families=LONG_FAMILIES),
    _v("f32-d40-two-kernel-long", "flash_f32", 1, 1, 2, 1100, 1100, 40, "q128", ("two_kernel", 1),
       tune={"fa2_two_kernel_bwd": 1}, families=LONG_FAMILIES),
    _v("f32-d80-two-kernel-long", "flash_f32", 1, 1, 2, 1100, 1100, 80, "q128", ("two_kernel", 1),
       tune={"fa2_two_kernel_bwd": 1}, families=LONG_FAMILIES),
    # ---- flash, split bf16.  fwd: "w16" / "w32" queries per wave; the backward exists for d = 40 self-attention only
    _v("split-d40-w16-shared", "flash_split", 2, 1, 2, 130, 200, 40, "w16"),
    _v("split-d80-w16-shared", "flash_split", 2, 1, 2, 130, 200, 80, "w16"),
    _v("split-d40-w32-shared", "flash_split", 32, 1, 8, 70, 130, 40, "w32"),
    _v("split-d80-w32-shared", "flash_split", 32, 1, 8, 70, 130, 80, "w32"),
    _v("split-d40-bwd-77", "flash_split", 2, 2, 2, 77, 77, 40, "w16", ("split", 1)),
    _v("split-d40-bwd-300", "flash_split", 2, 2, 2, 300, 300, 40, "w16", ("split", 1)),
    # ---- cross-attention, <= 128 keys held in registers.  The form is the forward's and the backward's alike
    _v("cross-d8-T77", "cross", 2, 1, 2, 130, 77, 8, "ca_plain", "ca_plain"),
    _v("cross-d8-T128", "cross", 2, 2, 2, 130, 128, 8, "ca_plain", "ca_plain"),
    _v("cross-d40-T20", "cross", 2, 1, 2, 130, 20, 40, "ca_plain", "ca_plain"),
    _v("cross-d40-T77", "cross", 2, 1, 2, 130, 77, 40, "ca_plain", "ca_plain"),
    _v("cross-d40-T128", "cross", 2, 2, 2, 130, 128, 40, "ca_plain", "ca_plain"),
    _v("cross-d64-T77", "cross", 2, 1, 2, 130, 77, 64, "ca_plain", "ca_plain"),
    _v("cross-d64-T128", "cross", 2, 2, 2, 130, 128, 64, "ca_plain", "ca_plain"),
    _v("cross-d80-ts-T40", "cross", 1, 1, 3, 96, 40, 80, "ca_token_split", "ca_token_split"),
    _v("cross-d80-ts-T77", "cross", 2, 1, 2, 130, 77, 80, "ca_token_split", "ca_token_split"),
    _v("cross-d160-ts-T40", "cross", 1, 1, 3, 96, 40, 160, "ca_token_split", "ca_token_split"),
    _v("cross-d160-ts-T128", "cross", 2, 2, 2, 130, 128, 160, "ca_token_split", "ca_token_split"),
    _v("cross-d80-plain-forced", "cross", 2, 1, 2, 130, 77, 80, "ca_plain", "ca_plain", tune={"cross_attn_ts": 1}),
    # ---- first-generation head sizes behind the flash entry (the dense backward entry)
    _v("gen1-d8", "gen1", 2, 1, 2, 100, 131, 8, "self_attn_gen1", "self_attn_gen1"),
    _v("gen1-d16", "gen1", 2, 1, 2, 100, 131, 16, "self_attn_gen1", "self_attn_gen1"),
    _v("gen1-d32", "gen1", 2, 1, 2, 100, 131, 32, "self_attn_gen1", "self_attn_gen1"),
    _v("gen1-d32-own", "gen1", 2, 2, 2, 100, 131, 32, "self_attn_gen1", "self_attn_gen1"),
]


# ---------------------------------------------------------------------------------------------------------------------
# the launch plans, restated from the sources (a change there must be repeated here, and in _attn_cases.VARIANTS)
# ---------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def flash_fwd_plan(B, Bk, H, N, Nk, d):
    """csrc/skp_flash_attn.hip, skp_fa2_fwd"""
    if d == 160:
        return "d160_halves" if Nk >= 4 * 32 and _cdiv(N, 64) * H * B <= 1024 else "d160"
    return "q256" if d == 40 and _cdiv(N, 256) * H * B >= 512 else "q128"


def split_fwd_plan(B, Bk, H, N, Nk, d):
    """csrc/skp_flash_attn_s.hip, skp_flash_attn_fwd_split_f32"""
    return "w16" if _cdiv(N, 256) * H * B < 256 else "w32"


def flash_bwd_plan(B, Bk, H, N, Nk, d, two_kernel_forced):
    """csrc/skp_flash_attn.hip, fa2_fused_ok / fa2_fused_splits / fa2_two_kernel_splits / skp_fa2_bwd_workspace
    -> (form, splits), bytes of workspace"""
    floats = B * H * N
    fused = (not two_kernel_forced and d in (40, 64, 80) and Bk == B and N == Nk and N >= 1024
             and _cdiv(Nk, 128) * B * N * H * d * 4 <= 2 << 30)
    if fused:
        ns = 2 if d == 80 and _cdiv(Nk, 128) * H * B * 2 <= 256 and N >= 256 else 1
        floats += _cdiv(Nk, 128) * B * N * H * d + (ns * 2 * B * Nk * H * d if ns > 1 else 0)
        return ("fused", ns), 4 * floats
    ns = 1
    if d == 160:
        wgs, tiles = _cdiv(max(N, Nk), 64) * H * B, min(N, Nk) // 32
        while ns < 4 and wgs * ns * 2 <= 256 and tiles // (ns * 2) >= 2:
            ns *= 2
    floats += ns * B * (N + 2 * Nk) * H * d if ns > 1 else 0
    return ("two_kernel", ns), 4 * floats


def assert_plan(ops, v):
    """The shape of variant `v` reaches the plan it is listed for (call it with the variant's overrides set)."""
    lib, shape, kern = ops.N.lib(), v["shape"], v["kernel"]
    B, Bk, H, N, Nk, d = shape
    if kern == "flash_f32":
        assert d in ops.FA2_HEAD_DIMS and flash_fwd_plan(*shape) == v["fwd"]
        plan, nbytes = flash_bwd_plan(*shape, lib.skp_tune_get(b"fa2_two_kernel_bwd") == 1)
        assert plan == v["bwd"], (plan, v["bwd"])
        assert lib.skp_flash_attn_bwd_workspace(*shape) == nbytes, "the library plans another backward form for this shape"
    elif kern == "flash_split":
        assert lib.skp_flash_attn_fwd_split_ok(*shape) == 1 and split_fwd_plan(*shape) == v["fwd"]
        if v["bwd"]:
            assert lib.skp_flash_attn_bwd_split_ok(*shape) == 1
    elif kern == "cross":
        assert Nk <= ops.CROSS_ATTN_MAX_T
        form = ops.routes.cross_attn_form(B, H, N, Nk, d, lib.skp_tune_get(b"cross_attn_ts") == 1)
        assert form == v["fwd"] == v["bwd"], form
        if v["tune"].get("cross_attn_ts") == 1:               # the shape the override is there for
            assert ops.routes.cross_attn_form(B, H, N, Nk, d) == "ca_token_split"
    else:
        assert kern == "gen1" and d not in ops.FA2_HEAD_DIMS and d in ops.CROSS_ATTN_HEAD_DIMS
