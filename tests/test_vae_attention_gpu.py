"""The wide flash forward (one head of d = 512, csrc/skp_flash_attn_wide.hip) and the VAE attention route on the MI355X.

  * the kernel against fp64 on the hard-logit families of tests/_attn_cases.py, within  M_FLASH_WIDE x the error of the fp32
    MATERIALISED CPU reference (+1e-7), everything finite, same bits on a second call;
  * AttentionBlock(512) on the fused forward, flash route against library route, each against an fp64 host copy of the module,
    with the routes the ledger saw;
  * an input that needs a gradient keeps the library route and gets a finite gradient;
  * no N x N tensor is allocated at 8 192 keys;
  * a captured forward replays to the bits of the eager call.

Run with -s for one line per case: `attn-edge flash_wide <family> out: err, fp32ref, ratio` (profiles/attention_edges.md)."""
import copy

import pytest
import torch

import _attn_cases as A

pytestmark = pytest.mark.gpu

# err <= M x err_fp32ref + 1e-7: twice the largest ratio measured on the MI355X over the cases below, rounded up, and never above 8
# (the rule of _attn_cases.M; the measured ratios: profiles/attention_edges.md, row flash_wide)
M_FLASH_WIDE = 6          # largest ratio 2.71 ((2, 1, 17) spike_last)

TINY_FAMILIES = ("randn", "spike_last", "all_high", "all_low", "onehot", "tiny_scale")
SHAPES = [
    ((2, 1, 200), A.FAMILIES),           # ragged last tile, several tiles, two rows
    ((1, 2, 77), A.FAMILIES),            # two heads sharing a row's channels
    ((2, 1, 17), TINY_FAMILIES),         # one full 16-key tile and a tile of a single key
    ((1, 1, 9), ("randn", "all_high", "all_low", "onehot", "tiny_scale")),      # fewer keys than one tile
    ((1, 1, 1100), A.LONG_FAMILIES),     # 35 blocks of 32 keys, a running-maximum update on every one under ramp_up
]
CASES = [(shape, fam) for shape, fams in SHAPES for fam in fams]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


@pytest.mark.parametrize("shape,family", CASES, ids=[f"B{s[0]}H{s[1]}N{s[2]}-{f}" for s, f in CASES])
def test_kernel_vs_fp64_on_hard_logits(ops, shape, family):
    B, H, n = shape
    c = A.case(family, B, B, H, n, n, 512)
    holds, what = A.check_property(family, c.logits(), 512, c.scale)
    assert holds, f"{family} at {shape}: {what}"
    q, k, v = c.q.cuda(), c.k.cuda(), c.v.cuda()
    out = ops.flash_attn_wide(q, k, v, H, c.scale)
    again = ops.flash_attn_wide(q, k, v, H, c.scale)
    A.assert_attn_close({"out": out.cpu()}, c, M_FLASH_WIDE, "flash_wide")
    assert torch.equal(out, again)


def test_key_count_of_its_own_and_odd_scale(ops):
    """k / v with another row count than q (the C ABI takes both), a scale that is not 512^-1/2."""
    g = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(2, 70, 512, generator=g), torch.randn(2, 45, 512, generator=g), torch.randn(2, 45, 512, generator=g)
    scale = 0.0625

    def ref(dt):
        return torch.softmax((q.to(dt) @ k.to(dt).transpose(1, 2)) * scale, dim=-1) @ v.to(dt)
    r64 = ref(torch.float64)
    e32 = A.rel_err(ref(torch.float32), r64)
    err = A.rel_err(ops.flash_attn_wide(q.cuda(), k.cuda(), v.cuda(), 1, scale).cpu(), r64)
    print(f"flash_wide Nk != N: err {err:.3e} fp32ref {e32:.3e}")
    assert err <= M_FLASH_WIDE * e32 + A.ABS_SLACK


# ---------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block():
    """(fused AttentionBlock(512) on the GPU, its fp64 copy on the host), seeded weights, frozen as the VAE is."""
    from stablekeypoints_amd.ldm.attention import AttentionBlock
    from stablekeypoints_amd.ldm.fused import fuse_norms
    torch.manual_seed(11)
    m = AttentionBlock(512)
    with torch.no_grad():
        m.group_norm.weight.normal_(1.0, 0.2)
        m.group_norm.bias.normal_(0.0, 0.2)
    m.requires_grad_(False)
    m64 = copy.deepcopy(m).double()
    m = m.cuda()
    fuse_norms(m)
    assert "forward" in m.__dict__
    return m, m64


def _x(seed=5):
    return torch.randn(2, 512, 24, 24, generator=torch.Generator().manual_seed(seed))


def test_module_parity_and_routes(ops, block, monkeypatch):
    from stablekeypoints_amd import routes
    m, m64 = block
    x = _x()
    with torch.no_grad():
        ref = m64(x.double())
        monkeypatch.setattr(ops, "VAE_ATTN_MODE", "flash")
        before = routes.snapshot()
        with routes.expect():
            y_flash = m(x.cuda())
        d = routes.delta(before)
        assert d.get(("vae.attention", "flash_wide"), 0) == 1 and d.get(("vae.attention", "lib_core"), 0) == 0, d
        monkeypatch.setattr(ops, "VAE_ATTN_MODE", "lib")
        before = routes.snapshot()
        y_lib = m(x.cuda())
        assert routes.delta(before).get(("vae.attention", "lib_core"), 0) == 1
        monkeypatch.setattr(ops, "VAE_ATTN_MODE", "auto")
        before = routes.snapshot()
        y_auto = m(x.cuda())
        d = routes.delta(before)
        assert d.get(("vae.attention", "lib_core"), 0) == 1 and d.get(("vae.attention", "flash_wide"), 0) == 0, d
    e_flash, e_lib = A.rel_err(y_flash.cpu(), ref), A.rel_err(y_lib.cpu(), ref)
    print(f"AttentionBlock(512) at 576 keys vs fp64: flash {e_flash:.3e} lib {e_lib:.3e}")
    assert torch.isfinite(y_flash).all()
    assert e_flash <= 4 * e_lib + 1e-7
    assert torch.equal(y_auto, y_lib)


def test_gradient_keeps_the_library_route(ops, block, monkeypatch):
    from stablekeypoints_amd import routes
    m, _ = block
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", "flash")
    x = _x(6).cuda().requires_grad_(True)
    before = routes.snapshot()
    y = m(x)
    d = routes.delta(before)
    assert d.get(("vae.attention", "lib_core"), 0) == 1 and d.get(("vae.attention", "flash_wide"), 0) == 0, d
    y.square().mean().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    with torch.no_grad():                                   # the same input without grad mode is free to take the kernel
        before = routes.snapshot()
        m(x)
        assert routes.delta(before).get(("vae.attention", "flash_wide"), 0) == 1


def test_no_quadratic_memory(ops):
    n = 8192
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(1, n, 512, generator=g) for _ in range(3))
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    scale = 512 ** -0.5
    ws = int(ops.N.lib().skp_flash_attn_fwd_wide_workspace(1, 1, 1, n, n, 512))
    ops.flash_attn_wide(qd[:, :64], kd[:, :64], vd[:, :64], 1, scale)                 # the kernel's one-time set-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.flash_attn_wide(qd, kd, vd, 1, scale)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    out_bytes = n * 512 * 4
    print(f"flash_wide at {n} keys: peak allocation {peak / 2**20:.1f} MiB over the call (out {out_bytes / 2**20:.1f} MiB, "
          f"workspace {ws} B; one score matrix would be {n * n * 4 / 2**20:.0f} MiB)")
    assert ws >= 0 and peak < n * n * 4 // 2 and peak <= out_bytes + ws + (2 << 20)
    rows = torch.randperm(n, generator=g)[:64]

    def ref(dt):
        return torch.softmax((q[0, rows].to(dt) @ k[0].to(dt).T) * scale, dim=-1) @ v[0].to(dt)
    r64 = ref(torch.float64)
    e32 = A.rel_err(ref(torch.float32), r64)
    err = A.rel_err(out[0].cpu()[rows], r64)
    print(f"flash_wide at {n} keys, 64 sampled rows: err {err:.3e} fp32ref {e32:.3e}")
    assert torch.isfinite(out).all() and err <= M_FLASH_WIDE * e32 + A.ABS_SLACK


def test_captured_replay_is_bitwise(ops, block, monkeypatch):
    m, _ = block
    monkeypatch.setattr(ops, "VAE_ATTN_MODE", "flash")
    xs = [_x(21).cuda(), _x(22).cuda()]
    with torch.no_grad():
        eager = [m(x) for x in xs]
        static = xs[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(static)
        for x, want in zip(xs, eager):
            static.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, want)
