"""The attention core against fp64 on inputs that make the online softmax work (tests/_attn_cases.py): flash fp32, flash split
bf16, short-key cross-attention and the first-generation head sizes, every launch plan of each, on every input family.

Per case (kernel variant x family):
  * out, lse (natural log), dq, dk, dv within  M[kernel family] x the error of the fp32 MATERIALISED CPU reference  (+1e-7) of
    fp64, everything finite;
  * dk / dv of a shared k / v row by row, as the C ABI writes them ([B,Nk,C]), not only summed;
  * a second call gives the same bits;
  * the launch plan the shape was chosen for is the one that ran: the route ledger for the kernel family, the library's
    workspace query for the backward form (fused / two kernels, number of range splits), `routes.cross_attn_form` for
    cross-attention.  The forward plans have no query; their gates are restated below and the table of variants is checked
    against the restatement.
Per variant, on spike_last: every tensor inside NaN guard bands, the workspace exactly the queried size: same bits, guards
untouched.

Run with -s for one line per output: `attn-edge <variant> <family> <output>: err, fp32ref, ratio` (profiles/attention_edges.md)."""
import math
import time

import pytest
import torch

import _attn_cases as A

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of guard band on each side (256 bytes: the interior keeps its 16-byte alignment)
GUARD_BITS = 0x7FC0BEEF         # a NaN with a payload no kernel produces


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def expected_ledger(v):
    route = {"flash_f32": "flash_f32", "flash_split": "flash_split", "gen1": "self_attn_gen1"}.get(v["kernel"])
    if route is None:
        return {}                                             # cross-attention is launched through the C ABI: nothing notes
    led = {("flash.fwd", route): 1}
    if v["bwd"] and v["kernel"] != "gen1":                    # (gen1: the dense backward entry, through the C ABI)
        led[("flash.bwd", route)] = 1
    return led


# ---------------------------------------------------------------------------------------------------------------------
# launching a variant
# ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """Device tensors of one launch, outputs pre-filled with NaN; `guarded`: each in the interior of its own larger buffer
    with GUARD floats of a marked NaN on both sides."""

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
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        return t

    def put(self, t):
        return self.empty(*t.shape).copy_(t)

    def workspace(self, nbytes):
        assert nbytes >= 0 and nbytes % 4 == 0
        return self.empty(nbytes // 4) if nbytes else None

    def intact(self):
        return all(bool((b.view(torch.int32)[:GUARD] == GUARD_BITS).all()) and bool((b.view(torch.int32)[GUARD + n:] == GUARD_BITS).all())
                   for b, n in self.bufs)


def run_variant(ops, v, c, arena):
    """Forward (and backward from the forward's own out / lse) of variant `v` on case `c` -> name -> device tensor.  An error of the
    HIP runtime (a failed launch, a fault reported at the synchronisation) ends the session: nothing more may start on that device."""
    try:
        return _run_variant(ops, v, c, arena)
    except RuntimeError as e:
        if "hip" in str(e).lower():
            pytest.exit(f"{v['name']} on {c.family}: {e}", returncode=3)
        raise


def _run_variant(ops, v, c, arena):
    lib, kern = ops.N.lib(), v["kernel"]
    B, Bk, H, N, Nk, d = v["shape"]
    C, st = H * d, ops._stream()
    q, k, vv, g = (arena.put(t) for t in (c.q, c.k, c.v, c.dout))
    out, lse = arena.empty(B, N, C), arena.empty(B, H, N)
    if kern == "cross":
        ops.N.check(lib.skp_cross_attn_fwd_f32(q.data_ptr(), k.data_ptr(), vv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                               B, Bk, H, N, Nk, d, c.scale, st), "skp_cross_attn_fwd_f32")
    else:
        ops._flash_fwd(q, k, vv, out, lse, H, c.scale, split=kern == "flash_split")
    res = {"out": out, "lse": lse}
    if v["bwd"]:
        dq, dk, dv = arena.empty(B, N, C), arena.empty(B, Nk, C), arena.empty(B, Nk, C)      # dk / dv: B rows even for a shared k / v
        ptrs = (q.data_ptr(), k.data_ptr(), vv.data_ptr(), out.data_ptr(), g.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                dk.data_ptr(), dv.data_ptr())
        if kern == "cross":
            ws = arena.workspace(lib.skp_cross_attn_bwd_workspace(B, H, N, Nk, d))
            ops.N.check(lib.skp_cross_attn_bwd_f32(*ptrs, ws.data_ptr(), B, Bk, H, N, Nk, d, c.scale, st), "skp_cross_attn_bwd_f32")
        elif kern == "gen1":
            ws = arena.workspace(lib.skp_flash_attn_bwd_workspace(B, Bk, H, N, Nk, d))
            ops.N.check(lib.skp_flash_attn_bwd_f32(*ptrs, ws.data_ptr(), B, Bk, H, N, Nk, d, c.scale, st), "skp_flash_attn_bwd_f32")
        else:
            ops._flash_bwd(q, k, vv, out, g, lse, H, c.scale, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), C, split=kern == "flash_split")
        res.update(dq=dq, dk=dk, dv=dv)
    torch.cuda.synchronize()
    return res


def _id(v):
    return v["name"]


CASES = [(v, f) for v in A.VARIANTS for f in v["families"]]


def test_every_family_that_must_run_does():
    must = {"spike_last", "ramp_up", "all_high", "all_low", "odd_scale"}
    for v in A.VARIANTS:
        assert must <= set(v["families"]), v["name"]
        B, Bk, H, N, Nk, d = v["shape"]
        ragged = N % 64 != 0 and Nk % 64 != 0
        assert ragged or (N, Nk) == (1024, 1024) or (v["kernel"] == "cross" and Nk == 128), v["name"]    # sizes the issue names


@pytest.mark.parametrize("v,family", CASES, ids=[f"{v['name']}-{f}" for v, f in CASES])
def test_attention_kernel_vs_fp64(ops, tune, v, family):
    for key, value in v["tune"].items():
        tune(key, value)
    A.assert_plan(ops, v)
    t0 = time.perf_counter()
    c = A.case(family, *v["shape"])
    ops.routes.reset()
    first = run_variant(ops, v, c, Arena(False))
    assert ops.routes.snapshot() == expected_ledger(v), ops.routes.table()
    second = run_variant(ops, v, c, Arena(False))
    A.assert_attn_close({name: t.cpu() for name, t in first.items()}, c, A.M[v["kernel"]], v["name"])
    for name in first:
        assert torch.equal(first[name], second[name]), f"{v['name']} {family}: {name} differs between two calls"
    print(f"attn-edge-time {v['name']} {family}: {time.perf_counter() - t0:.2f} s  fwd {v['fwd']} bwd {v['bwd']}")


@pytest.mark.parametrize("v", A.VARIANTS, ids=_id)
def test_attention_kernel_stays_inside_its_buffers(ops, tune, monkeypatch, v):
    """spike_last (the hot key in the ragged tail tile) with every tensor between NaN guard bands and the workspace exactly as
    large as its query says: bit-equal to the plain call, every guard untouched.  A kernel that reads a row past N / Nk and
    counts on 0 * x to drop it, or writes past a ragged tile, fails here.  Every byte touched lies inside a torch allocation."""
    for key, value in v["tune"].items():
        tune(key, value)
    A.assert_plan(ops, v)
    c = A.case("spike_last", *v["shape"])
    plain = run_variant(ops, v, c, Arena(False))
    arena = Arena(True)
    lib = ops.N.lib()
    sizes = []

    def exact_workspace(query, *args, device):
        sizes.append(int(getattr(lib, query)(*args)))
        return arena.workspace(sizes[-1])
    monkeypatch.setattr(ops, "_workspace", exact_workspace)
    guarded = run_variant(ops, v, c, arena)
    if v["kernel"] == "flash_f32":
        assert sizes == [A.flash_bwd_plan(*v["shape"], v["tune"].get("fa2_two_kernel_bwd") == 1)[1]]
    for name in plain:
        assert torch.isfinite(guarded[name]).all(), name
        assert torch.equal(plain[name], guarded[name]), f"{v['name']}: {name} changes when its neighbourhood is NaN"
    assert arena.intact(), f"{v['name']}: a guard band was written"
