"""The attention-map kernels against fp64 on logits that make them work (tests/_map_cases.py): the fused, grouped and wide
forward, the dense, grouped, column-sweep and token-major-sweep backward, and the fp32-MFMA GEMMs around them, every launch plan
of each, on every logit family.

Per case (variant x family):
  * M, lse (log2 units) and every dS_l (or dq_l / dk_l) within  M[route] x the error of the fp32 CPU reference  (+1e-7) of fp64,
    everything finite; pad columns of dS exactly 0; M sums to 1 over tokens within 1e-5;
  * a second call gives the same bits;
  * the route ledger shows exactly the expected ("map.fwd", ...) / ("map.bwd", ...) pair;
  * wide forward: a row selection with a repeated and an unsorted index equals the gathered full result, bit for bit.
Per variant, on spike_last: every input, output and workspace inside NaN-payload guard bands, the workspace exactly the queried
size, launched through `ops._launch`: same bits as the unguarded run, guards untouched.

Run with -s for one line per output: `map-edge <variant> <family> <output>: err, fp32ref, ratio` (profiles/map_edges.md)."""
import math

import pytest
import torch

import _map_cases as A

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of guard band on each side (256 bytes: the interior keeps its 32-byte alignment)
GUARD_BITS = 0x7FC0BEEF         # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


@pytest.fixture
def configured(ops, monkeypatch, tune):
    """-> set(v): the module switches and library overrides of variant `v`, undone after the test; `_stack_grads` hands back the
    logits gradient instead of going on to the GEMMs (the q, k variants take the real one)."""
    def set_(v):
        monkeypatch.setattr(ops, "MAP_WIDE", v["wide"])
        monkeypatch.setattr(ops, "MAP_BWD_MODE", v["mode"])
        for key, value in v["tune"].items():
            tune(key, value)
        if v["kind"] == "S":
            monkeypatch.setattr(ops, "_dqk_from_dS", lambda qs, ks, dS, scales, H, T, needs: dS)
    return set_


def _guarded_call(v, family, fn, *args):
    """An error of the HIP runtime (a failed launch, a fault reported at the synchronisation) ends the session: nothing more may
    start on that device."""
    try:
        out = fn(*args)
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit(f"{v['name']} on {family}: {e}", returncode=3)
        raise


def _stack(ops, v):
    """The geometry of a stack whose logits are given (no q, k: `_dqk_from_dS` is replaced for these variants)."""
    L = len(v["sides"])
    return ops.MapStack._make(((), (), v["H"], (1.0,) * L, v["R"], v["sides"], v["B"], v["B"], v["T"], L))


def _run(ops, v, c):
    """Forward and backward of variant `v` on case `c` through the three functions every route is behind -> (name -> device
    tensors, the ledger's additions)."""
    sides, H, T, R, B = v["sides"], v["H"], v["T"], v["R"], v["B"]
    L = len(sides)
    if v["kind"] == "S":
        S = [s.cuda() for s in c.S]
        before = ops.routes.snapshot()
        M, lse = ops._map_fwd(S, sides, B, H, T, R)
        grad = dict(rows=(c.sel.cuda(), c.G.cuda())) if v["rows"] else dict(dM=c.dM.cuda())
        dS = ops._stack_grads(_stack(ops, v), S, lse, (True,) * (2 * L), **grad)
        return {"M": M, "lse": lse, "dS": dS}, ops.routes.delta(before)
    qs = [q.cuda().requires_grad_(True) for q in c.qs]
    ks = [k.cuda().requires_grad_(True) for k in c.ks]
    with torch.no_grad():
        lse = ops.MapStack("map edges", qs, ks, H, c.scales, R).maps()[2]
    before = ops.routes.snapshot()
    M = ops.attn_map(qs, ks, H, c.scales, R)
    M.backward(c.dM.cuda())
    return {"M": M.detach(), "lse": lse, "dq": [q.grad for q in qs], "dk": [k.grad for k in ks]}, ops.routes.delta(before)


def _same_bits(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("v,family", A.CASES, ids=[f"{v['name']}-{f}" for v, f in A.CASES])
def test_map_routes_vs_fp64_on_hard_logits(ops, configured, v, family):
    T = v["T"]
    c = A.case(v, family)
    configured(v)
    A.assert_plan(ops, v)
    out, ledger = _guarded_call(v, family, _run, ops, v, c)
    assert ledger == {("map.fwd", v["fwd"]): 1, ("map.bwd", v["bwd"]): 1}, ledger
    got = {k: ([t[..., :T].cpu() for t in x] if k == "dS" else [t.cpu() for t in x] if isinstance(x, list) else x.cpu())
           for k, x in out.items()}
    A.assert_map_close(got, c, "kernel")
    assert (got["M"].sum(1) - 1).abs().max().item() <= 1e-5
    if "dS" in out:
        assert all(d.shape[-1] == A.nt_of(T) and not d[..., T:].any() for d in out["dS"]), "pad columns of dS must be exactly 0"
    again, _ = _guarded_call(v, family, _run, ops, v, c)
    assert all(_same_bits(out[k], again[k]) for k in out), "a second call gives other bits"
    if v["tokrow"]:
        S = [s.cuda() for s in c.S]
        idx = torch.tensor([T - 1, 0, 5, 0, T // 2], device="cuda")                   # unsorted, token 0 twice
        uniq, inv = torch.unique(idx, return_inverse=True)                             # as ops.attn_map_rows does
        tokrow = torch.full((T,), -1, device="cuda", dtype=torch.int32)
        tokrow[uniq] = torch.arange(uniq.numel(), device="cuda", dtype=torch.int32)
        Msel, lse = _guarded_call(v, family, lambda: ops._map_fwd(S, v["sides"], v["B"], v["H"], T, v["R"], tokrow=tokrow, n_rows=int(uniq.numel())))
        assert Msel.shape[1] == 4 and _same_bits(Msel[:, inv], out["M"][:, idx]) and _same_bits(lse, out["lse"])


# ---------------------------------------------------------------------------------------------------------------------
# the same launches with every buffer between guard bands
# ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """Device tensors of one launch, outputs pre-filled with NaN; `guarded`: each in the interior of its own larger buffer with
    GUARD floats of a marked NaN on both sides."""

    def __init__(self, guarded):
        self.guarded, self.bufs = guarded, []

    def empty(self, *shape):
        n = math.prod(shape)
        if not self.guarded:
            return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)
        buf = torch.empty(n + 2 * GUARD, device="cuda", dtype=torch.float32)
        buf.view(torch.int32).fill_(GUARD_BITS)
        self.bufs.append((buf, n))
        t = buf[GUARD:GUARD + n].view(shape)
        assert t.data_ptr() % 32 == 0 and t.is_contiguous()
        return t

    def put(self, t):
        if t.dtype == torch.int64:                            # the selected rows: two floats of room per index
            return self.empty(*t.shape, 2).view(torch.int64).view(t.shape).copy_(t)
        return self.empty(*t.shape).copy_(t)

    def workspace(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return self.empty(nbytes // 4)

    def intact(self):
        return all(bool((b.view(torch.int32)[:GUARD] == GUARD_BITS).all()) and bool((b.view(torch.int32)[GUARD + n:] == GUARD_BITS).all())
                   for b, n in self.bufs)


def _launch_variant(ops, v, c, arena):
    """The launches `ops.qk_logits` / `_map_fwd` / `_map_bwd` / `_map_bwd_sparse` / `_dqk_from_dS` make for variant `v`, through
    `ops._launch` with every tensor from `arena` and the workspace exactly as large as the library's query says."""
    N, lib = ops.N, ops.N.lib()
    sides, H, T, R, B, K = v["sides"], v["H"], v["T"], v["R"], v["B"], v["K"]
    L, ldt, RR = len(sides), A.nt_of(T), R * R
    if v["kind"] == "qk":                                     # the logits by the fp32-MFMA GEMM (it writes the pad columns as 0)
        Bk, d = v["Bk"], v["d"]
        qs, ks = [arena.put(q.cuda()) for q in c.qs], [arena.put(k.cuda()) for k in c.ks]
        S = [arena.empty(B, H, s * s, ldt) for s in sides]
        for q, k, S_l, sc, s in zip(qs, ks, S, c.scales, sides):
            ops._launch("skp_qk_logits_f32", q, k, S_l, B, Bk, H, T, s * s, d, float(sc))
    else:
        S = [arena.put(s.cuda()) for s in c.S]
    si, _k0 = N.int_array(sides)
    M, lse = arena.empty(B, T, R, R), arena.empty(B, L * H, RR)

    def ptrs(ts, t0=0):
        return N.ptr_array([t.data_ptr() + 4 * t0 for t in ts])

    def fwd(t0, t1, mode, lse_out, lse_in):
        sp, _k = ptrs(S, t0)
        ops._launch("skp_attn_map_fwd_ex_f32", sp, si, L, B, H, t1 - t0, R, M.data_ptr() + 4 * t0 * RR, lse_out, lse_in, ldt, T * RR, mode)

    if v["fwd"] == "map_wide":
        sp, _k = ptrs(S)
        ops._launch("skp_attn_map_fwd_wide_f32", sp, si, L, B, H, T, R, M, lse, None, 0, ldt)
    elif v["fwd"] == "map_fused":
        fwd(0, T, 0, lse, None)
    else:
        parts = [arena.empty(B, L * H, RR) for _ in A.groups(T)]
        for (t0, t1), part in zip(A.groups(T), parts):
            fwd(t0, t1, 1, part, None)
        lse.copy_(ops._log2sumexp2(parts))
        for t0, t1 in A.groups(T):
            fwd(t0, t1, 2, None, lse)
    out = {"M": M, "lse": lse}
    if v["bwd"] in ("map_dense", "map_dense_groups"):
        if v["rows"]:
            sel, G = c.sel.cuda(), c.G.cuda()
            dM = arena.put(torch.zeros(B, T, R, R, device="cuda").scatter_(1, sel[:, :, None, None].expand_as(G), G))
        else:
            dM = arena.put(c.dM.cuda())
        dS = [arena.empty(*s.shape) if T <= A.TOKEN_GROUP else arena.put(torch.zeros_like(s)) for s in S]
        Tl = T if T <= A.TOKEN_GROUP else A.GROUP_STEP
        ws = arena.workspace(lib.skp_attn_map_bwd_workspace(si, L, B, H, Tl, R))

        def bwd(t0, t1, mode, dot):
            sp, _k1 = ptrs(S, t0)
            dp, _k2 = ptrs(dS, t0)
            ops._launch("skp_attn_map_bwd_ex_f32", sp, dp, si, L, B, H, t1 - t0, R, dM.data_ptr() + 4 * t0 * RR, lse, ws, dot, ldt, T * RR, mode)

        if T <= A.TOKEN_GROUP:
            bwd(0, T, 0, None)
        else:
            dots = [arena.empty(B, L * H, RR) for _ in A.groups(T)]
            for (t0, t1), d in zip(A.groups(T), dots):
                bwd(t0, t1, 1, d)
            dot = arena.put(torch.stack(dots, 0).sum(dim=0))
            for t0, t1 in A.groups(T):
                bwd(t0, t1, 2, dot)
    else:
        col = v["bwd"] == "map_col"
        query = lib.skp_attn_map_bwd_col_workspace if col else lib.skp_attn_map_bwd_sparse_workspace
        ws = arena.workspace(query(si, L, B, H, T, R, K))
        sel, G = arena.put(c.sel.cuda()), arena.put(c.G.cuda())
        dS = [arena.empty(*s.shape) for s in S]
        sp, _k1 = ptrs(S)
        dp, _k2 = ptrs(dS)
        ops._launch("skp_attn_map_bwd_col_f32" if col else "skp_attn_map_bwd_sparse_f32", sp, dp, si, L, B, H, T, R, sel, G, K, lse, ws, ldt)
    out["dS"] = dS
    if v["kind"] == "qk":                                     # dq, dk as ops._dqk_from_dS forms them; a shared k sums over the batch
        C = H * d
        out["dq"], out["dk"] = [], []
        for q, k, ds, sc, s in zip(qs, ks, dS, c.scales, sides):
            s2 = s * s
            dq, dkb = arena.empty(B, s2, C), arena.empty(B, T, C)
            ops._gemm_nt(ds, k, dq, s2, d, T, B, H, (H * s2 * ldt, s2 * ldt, ldt, 1), (0 if Bk == 1 else T * C, d, 1, C), (s2 * C, d, C), sc)
            ops._gemm_nt(ds, q, dkb, T, d, s2, B, H, (H * s2 * ldt, s2 * ldt, 1, ldt), (s2 * C, d, 1, C), (T * C, d, C), sc)
            out["dq"].append(dq)
            out["dk"].append(dkb.sum(dim=0, keepdim=True) if Bk == 1 and B > 1 else dkb)
    return out


@pytest.mark.parametrize("v", A.VARIANTS, ids=[v["name"] for v in A.VARIANTS])
def test_map_launches_stay_inside_their_buffers(ops, configured, v):
    family = "spike_last"
    c = A.case(v, family)
    configured(v)
    plain = _guarded_call(v, family, _launch_variant, ops, v, c, Arena(False))
    arena = Arena(True)
    guarded = _guarded_call(v, family, _launch_variant, ops, v, c, arena)
    assert arena.intact(), "a kernel wrote outside one of its buffers"
    assert all(_same_bits(plain[k], guarded[k]) for k in plain), "the guarded run gives other bits"
    assert all(A._finite(x) for x in guarded.values()), "an output element was left unwritten"
    via_ops, _ = _guarded_call(v, family, _run, ops, v, c)
    assert all(_same_bits(via_ops[k], guarded[k]) for k in via_ops), "ops takes another launch sequence than restated here"
