"""Keypoint guidance on the MI355X: the point-loss kernel and the step kernel's gradient term against fp64 with derived per-element
bounds, `ops.MapPointLossFn` and `ptp_utils.keypoint_energy_grad` against the fp64 host formula (held to the error of the route the
package had before: dense fused maps, a gather and a torch MSE under autograd), and `text2image_ldm_stable(keypoints=...)` against
the fp64 host loop of tests/_keypoint_cases.py.  The measured figures are recorded in profiles/generate_keypoints.md."""
import itertools

import pytest
import torch

import _keypoint_cases as C

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def _rel(a, ref):
    return ((a.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the point-loss kernel
# ---------------------------------------------------------------------------------------------------------------------------------
# Roundings into G, each at most 2^-24 of |M| + |t|.  t = expf(-a_hi) (1 - a_lo), the exponent formed in fp64 and split into two
# floats: expf's documented error of 1 ulp = 2 units, the difference 1 - a_lo 1, the product 1 (the first-order factor is off by
# a_lo^2 / 2 < 2^-37 and the fp64 exponent by 2^-50 a: nothing) = 4 on t; the difference M - t 1; the coefficient 2 / (K R^2) rounded
# to a float 1 and the product with it 1: 7, rounded up to 8.  (Where t is below the normal range, under 2^-126, its absolute error
# of 2^-149 is no longer relative to t; the maps of these cases are not that small.)
U_G = 8.0
# The loss: d = M - t carries 5 of those units, d^2 therefore 2 * 5 + 1 = 11 units of (|M| + |t|)^2; 4 additions per lane, 6 of the
# wave's butterfly and 2 across the four waves are 12 roundings of partial sums that the sum of magnitudes bounds; the sum of the
# K * nchunk chunk sums (at most 528 here) in torch's reduction tree at most 16 more, the division by K R^2 1: 40.
U_E = 40.0


@pytest.mark.parametrize("B,K,R", [(1, 1, 16), (3, 3, 32), (2, 10, 40), (1, 33, 128)])
def test_point_loss_vs_fp64(ops, B, K, R):
    """R^2 below, equal to and ragged against the 1024-element chunk, K beyond 32; sigma 0.5 / 2 / 16; positions at corners, on
    pixel centres and outside the image; maps of softmax scale and of unit scale.  Per element |G - G64| <= 8 * 2^-24 (|M| + |t|) 2 /
    (K R^2), |E - E64| <= 40 * 2^-24 mean (|M| + |t|)^2; two calls give the same bits."""
    gen = torch.Generator().manual_seed(100 + R)
    special = torch.tensor([[0., 0.], [1., 1.], [0., 1.], [.5 / R, (R - .5) / R], [(R // 2 + .5) / R, (R // 3 + .5) / R], [-.25, .5],
                            [1.5, 1.125], [.3, -2.]])
    pos = torch.rand(B, K, 2, generator=gen)
    m = min(len(special), B * K)
    pos.reshape(-1, 2)[:m] = special[:m]
    worst_g = worst_e = 0.0
    for sigma, scale in itertools.product((0.5, 2.0, 16.0), (1.0 / 77, 1.0)):
        M = torch.rand(B, K, R, R, generator=gen) * scale
        E, G = ops.point_loss(M.cuda(), pos.cuda(), sigma)
        E2, G2 = ops.point_loss(M.cuda(), pos.cuda(), sigma)
        assert torch.equal(E, E2) and torch.equal(G, G2) and E.shape == (B,) and G.shape == M.shape
        M64 = M.double()
        E64, G64, t = C.energy_and_grad(M64, pos, sigma)
        mag = M64.abs() + t.abs()
        eg = (G.cpu().double() - G64).abs()
        assert (eg[mag == 0] == 0).all()                        # (a map element of exactly 0 under a target that underflowed)
        ug = (eg / (EPS * mag * 2 / (K * R * R)))[mag > 0].max().item()
        ue = ((E.cpu().double() - E64).abs() / (EPS * (mag ** 2).mean(dim=(1, 2, 3)))).max().item()
        worst_g, worst_e = max(worst_g, ug), max(worst_e, ue)
        assert ug <= U_G and ue <= U_E, (sigma, scale, ug, ue)
    print(f"point_loss B={B} K={K} R={R}: worst G error {worst_g:.2f} units (bound {U_G:.0f}), worst E error {worst_e:.2f} units "
          f"(bound {U_E:.0f})")


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the step kernel with the gradient term
# ---------------------------------------------------------------------------------------------------------------------------------
def _ref64(x, mc, mu, g, kind, clip, row, p, z, sg):
    """-> (y, S, x0, X0) in fp64: the formula of include/skp_keypoints.h, skp_sampler_step_kp_f32, and the magnitude sums its
    roundings are relative to (tests/test_samplers_gpu.py `_ref64` with the gradient term added to both).  `sg` = s g per element."""
    sa, sb, cx, c0, ce, c1, cn = row
    x, mc = x.double(), mc.double()
    if mu is None:
        m, M = mc, mc.abs()
    else:
        mu = mu.double()
        m, M = mu + g * (mc - mu), mu.abs() + abs(g) * (mc.abs() + mu.abs())
    ax = x.abs()
    if kind == 0:
        x0, eps, X0, E = (x - sb * m) / sa, m, (ax + sb * M) / sa, M
    elif kind == 1:
        x0, eps, X0, E = sa * x - sb * m, sa * m + sb * x, sa * ax + sb * M, sa * M + sb * ax
    else:
        x0, eps, X0, E = m, (x - sa * m) / sb, M, (ax + sa * M) / sb
    x0, eps, X0, E = x0 - (sb / sa) * sg, eps + sg, X0 + (sb / sa) * sg.abs(), E + sg.abs()
    if clip:
        x0 = x0.clamp(-1, 1)
    y, S = cx * x + c0 * x0 + ce * eps, abs(cx) * ax + abs(c0) * X0 + abs(ce) * E
    if p is not None:
        y, S = y + c1 * p.double(), S + abs(c1) * p.double().abs()
    if z is not None:
        y, S = y + cn * z.double(), S + abs(cn) * z.double().abs()
    return y, S, x0, X0


# The 16 of tests/test_samplers_gpu.py (14 counted there, rounded up) raised by the roundings the term adds: the product s g, the
# coefficient sb / sa rounded to a float, its product with s g, and the sum into x0 (or into eps): 4.
UNITS = 20.0


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [5, 1023, 16387])
def test_sampler_step_with_gradient_vs_fp64(ops, n, rows):
    """The case grid of test_sampler_step_vs_fp64 on [rows, n] elements (rows * n is odd: rows end inside a group of four lanes'
    elements), a scale per row: |y - y64| <= 20 * 2^-24 S and |x0_out - x0_64| <= 20 * 2^-24 X0 per element; copies = 2 gives the
    same bits twice; scales of zero give the bits of skp_sampler_step_f32."""
    from test_samplers_gpu import _step_rows
    gen = torch.Generator().manual_seed(300 + n + rows)
    scale = torch.tensor([0.1, 1.0, 4.0])[torch.arange(rows * n) % 3].reshape(rows, n)
    data = []
    for noise in (0.01, 1.0):
        x = torch.randn(rows, n, generator=gen) * scale
        mc = torch.randn(rows, n, generator=gen)
        mu = mc + noise * torch.randn(rows, n, generator=gen)
        p = torch.randn(rows, n, generator=gen) * scale.flip(1)
        z = torch.randn(rows, n, generator=gen)
        gr = torch.randn(rows, n, generator=gen) * 10.0 ** torch.randint(-3, 2, (rows, 1), generator=gen).float()
        s = torch.randn(rows, generator=gen) * 3
        data.append((noise, (x, mc, mu, p, z, gr, s), tuple(t.cuda() for t in (x, mc, mu, p, z, gr, s))))
    zero = torch.zeros(rows, device="cuda")
    worst, worst0, count = (0.0, None), (0.0, None), 0
    for (label, row), kind, clip, g, (has_p, has_z) in itertools.product(_step_rows(), (0, 1, 2), (False, True), (None, 7.5, 0.0, -2.0),
                                                                         ((True, True), (False, False), (True, False), (False, True))):
        noise, (x, mc, mu, p, z, gr, s), (xg, mcg, mug, pg, zg, grg, sg) = data[count % 2]
        count += 1
        row = tuple(row[:5]) + (row[5] if has_p else 0.0, row[6] if has_z else 0.0)
        kw = dict(x0_prev=pg if has_p else None, noise=zg if has_z else None, coef=row, guidance=1.0 if g is None else g,
                  prediction=kind, clip=clip)
        x0g = torch.empty(rows, n, device="cuda")
        y = ops.sampler_step(xg, mcg, None if g is None else mug, x0_out=x0g, grad=grg, grad_scale=sg, **kw)
        y2 = ops.sampler_step(xg, mcg, None if g is None else mug, copies=2, grad=grg, grad_scale=sg, **kw)
        assert y.shape == (rows, n) and y2.shape == (2 * rows, n)
        assert torch.equal(y2[:rows], y) and torch.equal(y2[rows:], y)
        x0z, x0p = torch.empty_like(x0g), torch.empty_like(x0g)
        assert torch.equal(ops.sampler_step(xg, mcg, None if g is None else mug, x0_out=x0z, grad=grg, grad_scale=zero, **kw),
                           ops.sampler_step(xg, mcg, None if g is None else mug, x0_out=x0p, **kw)) and torch.equal(x0z, x0p)
        ref, S, x0, X0 = _ref64(x, mc, None if g is None else mu, g, kind, clip, row, p if has_p else None, z if has_z else None,
                                s.double().reshape(rows, 1) * gr.double())
        where = (label, kind, clip, g, has_p, has_z, noise)
        units = ((y.cpu().double() - ref).abs() / (EPS * S)).max().item()
        units0 = ((x0g.cpu().double() - x0).abs() / (EPS * X0)).max().item()
        worst, worst0 = max(worst, (units, where)), max(worst0, (units0, where))
        assert units <= UNITS and units0 <= UNITS, (units, units0, where)
    print(f"sampler_step with gradient n={n} rows={rows}: worst y error {worst[0]:.2f} units of 2^-24 S at {worst[1]}; worst x0_out "
          f"error {worst0[0]:.2f} units of 2^-24 X0 at {worst0[1]} (bound {UNITS:.0f}; {count} cases)")


def test_sampler_step_with_gradient_aliasing_unaligned_and_determinism(ops):
    """The rules of the sibling entry, with the gradient present: two runs give the same bits; y may be x (or its first copy) and
    x0_out may be x0_prev; every pointer in turn one float past a 16-byte boundary -- `grad` among them -- takes the scalar form, held
    to the same bound."""
    from test_samplers_gpu import _step_rows
    rows, n = 3, 341                                            # 1023 elements
    gen = torch.Generator().manual_seed(23)
    x, mc, mu, p, z, gr = (torch.randn(rows, n, generator=gen).cuda() for _ in range(6))
    s = torch.tensor([1.5, -0.7, 0.02]).cuda()
    label, row = next((l, r) for l, r in _step_rows() if r[5] != 0 and r[6] != 0)
    for kind, clip in itertools.product((0, 1, 2), (False, True)):
        kw = dict(coef=row, guidance=7.5, prediction=kind, clip=clip, grad_scale=s)
        x0 = torch.empty(rows, n, device="cuda")
        y = ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, x0_out=x0, grad=gr, **kw)
        x0b = torch.empty(rows, n, device="cuda")
        assert torch.equal(y, ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, x0_out=x0b, grad=gr, **kw)) and torch.equal(x0, x0b)
        xa, pa = x.clone(), p.clone()
        assert ops.sampler_step(xa, mc, mu, x0_prev=pa, noise=z, out=xa, x0_out=pa, grad=gr, **kw) is xa
        assert torch.equal(xa, y) and torch.equal(pa, x0)
        buf, pa = torch.empty(2 * rows, n, device="cuda"), p.clone()
        buf[:rows] = x
        ops.sampler_step(buf[:rows], mc, mu, x0_prev=pa, noise=z, copies=2, out=buf, x0_out=pa, grad=gr, **kw)
        assert torch.equal(buf[:rows], y) and torch.equal(buf[rows:], y) and torch.equal(pa, x0)
        ref, S, r0, X0 = _ref64(x.cpu(), mc.cpu(), mu.cpu(), 7.5, kind, clip, row, p.cpu(), z.cpu(),
                                s.cpu().double().reshape(rows, 1) * gr.cpu().double())
        for which in range(8):                                  # x, m_c, m_u, x0_prev, noise, grad, y, x0_out
            t = [x, mc, mu, p, z, gr]
            if which < 6:
                base = torch.empty(rows * n + 1, device="cuda")
                base[1:] = t[which].reshape(-1)
                t[which] = base[1:].reshape(rows, n)
                assert t[which].data_ptr() % 16 == 4 and t[which].is_contiguous()
            out = torch.empty(rows * n + 1, device="cuda")[1:].reshape(rows, n) if which == 6 else None
            x0o = torch.empty(rows * n + 1, device="cuda")[1:].reshape(rows, n) if which == 7 else torch.empty(rows, n, device="cuda")
            yu = ops.sampler_step(t[0], t[1], t[2], x0_prev=t[3], noise=t[4], out=out, x0_out=x0o, grad=t[5], **kw)
            assert ((yu.cpu().double() - ref).abs() <= UNITS * EPS * S).all(), (kind, clip, which)
            assert ((x0o.cpu().double() - r0).abs() <= UNITS * EPS * X0).all(), (kind, clip, which)


def test_point_loss_far_positions(ops):
    """Positions so far outside the image that the exponent overflows a float: the target is 0 there, nothing is NaN, and E and G
    are those of a zero target."""
    gen = torch.Generator().manual_seed(3)
    M = torch.rand(1, 3, 16, 16, generator=gen).cuda()
    pos = torch.tensor([[[1e18, 0.5], [-3e30, 2e30], [0.5, 0.5]]]).cuda()
    E, G = ops.point_loss(M, pos, 0.5)
    assert torch.isfinite(E).all() and torch.isfinite(G).all()
    assert torch.equal(G[0, :2], M[0, :2] * torch.tensor(2.0 / (3 * 256)).float().cuda())
    E64, _, t = C.energy_and_grad(M.cpu().double(), pos.cpu(), 0.5)
    assert (t[0, :2] == 0).all() and t[0, 2].max() > 0.3
    assert ((E.cpu().double() - E64).abs() <= U_E * EPS * ((M.cpu().double() + t) ** 2).mean(dim=(1, 2, 3))).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. MapPointLossFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _host_energy64(qs, ks, heads, scales, R, ids, pos, sigma):
    """E [B] of the definitions in fp64 torch ops on the host (the host branch of `keypoint_energy_grad`, written out)."""
    from stablekeypoints_amd._maps import _materialize_host
    B = qs[0].shape[0]
    M = sum(_materialize_host(q, k, heads, sc, R).reshape(B, heads, R * R, -1)[..., ids].mean(dim=1) for q, k, sc in zip(qs, ks, scales))
    M = (M / len(qs)).permute(0, 2, 1).reshape(B, len(ids), R, R)
    return ((M - C.energy_and_grad(M.detach(), pos, sigma)[2]) ** 2).mean(dim=(1, 2, 3))


def _point_loss_case(ops, routes, sides, H, d, R, T, K, B, sigma, seed):
    """-> ((E error, dq error) of MapPointLossFn, the same of the older route, routes noted by the first), errors as max |delta| /
    max |ref| against the fp64 host formula on the same q / k."""
    from stablekeypoints_amd._maps import FusedAttn, fused_maps
    gen = torch.Generator().manual_seed(seed)
    scales = [d ** -0.5] * len(sides)
    qs = [torch.randn(B, s * s, H * d, generator=gen) for s in sides]
    ks = [torch.randn(1, T, H * d, generator=gen) for _ in sides]
    ids = sorted(torch.randperm(T, generator=gen)[:K].tolist())
    pos = torch.rand(B, K, 2, generator=gen)
    q64 = [q.double().requires_grad_() for q in qs]
    E64 = _host_energy64(q64, [k.double() for k in ks], H, scales, R, ids, pos, sigma)
    dq64 = torch.autograd.grad(E64.sum(), q64)
    E64 = E64.detach()

    def errors(E, dq):
        return _rel(E, E64), max(_rel(a, b) for a, b in zip(dq, dq64))

    qg = [q.cuda().requires_grad_() for q in qs]
    kg = [k.cuda() for k in ks]
    sel = torch.tensor(ids, device="cuda")
    tokrow = torch.full((T,), -1, dtype=torch.int32)
    tokrow[ids] = torch.arange(K, dtype=torch.int32)
    meta = dict(R=R, heads=H, scales=scales, sigma=sigma, pos=pos.cuda(), sel=sel, tokrow=tokrow.cuda())
    before = routes.snapshot()
    E = ops.MapPointLossFn.apply(meta, *[v for q, k in zip(qg, kg) for v in (q, k)])
    dq = torch.autograd.grad(E.sum(), qg)
    noted = routes.delta(before)
    new = errors(E, dq)
    # the route the package had before: dense fused maps under autograd, a gather, torch ops for the target and the MSE
    from stablekeypoints_amd.optimize_token import gaussian_circle
    Mo = fused_maps([FusedAttn(q, k, H, sc, R) for q, k, sc in zip(qg, kg, scales)])[:, sel]
    to = torch.stack([gaussian_circle(pos[b].cuda(), size=R, sigma=sigma) for b in range(B)])
    Eo = ((Mo - to) ** 2).mean(dim=(1, 2, 3))
    old = errors(Eo, torch.autograd.grad(Eo.sum(), qg))
    return new, old, noted


TINY = dict(sides=(4, 4, 4, 8), H=4, d=16, R=32, K=3, B=2, sigma=2.0)


@pytest.mark.parametrize("mode", ["auto", "sweep", "dense"])
@pytest.mark.parametrize("T", [16, 160])
def test_map_point_loss_fn_vs_fp64_tiny_shapes(ops, monkeypatch, mode, T):
    """The hooked layers of the reduced-width tree at 128^2 (sides 4, 4, 4, 8; 4 heads of 16 channels; R = 32) with 16 tokens and
    with 160 (the wide forward writes the K rows alone), under every map-backward mode: E and dq within 4x the error of the older
    route on the same inputs against the same fp64, and the ledger names the route."""
    from stablekeypoints_amd import routes
    monkeypatch.setattr(ops, "MAP_BWD_MODE", mode)
    new, old, noted = _point_loss_case(ops, routes, T=T, seed=7 + T, **TINY)
    print(f"MapPointLossFn tiny T={T} mode={mode}: E error {new[0]:.2e} (older route {old[0]:.2e}), dq error {new[1]:.2e} (older "
          f"route {old[1]:.2e})")
    want_bwd = {("auto", 16): "map_dense", ("auto", 160): "map_tok", ("sweep", 16): "map_tok", ("sweep", 160): "map_tok",
                ("dense", 16): "map_dense", ("dense", 160): "map_dense_groups"}[(mode, T)]
    assert noted.get(("map.bwd", want_bwd)) == 1 and noted.get(("map.fwd", "map_fused" if T == 16 else "map_wide")) == 1, noted
    assert new[0] <= 4 * old[0] and new[1] <= 4 * old[1], (new, old)


def test_map_point_loss_fn_vs_fp64_sd_shapes(ops):
    """sides (16, 16, 16, 32), 8 heads of 40 channels, R = 128, T = 77, K = 10, B = 2: the column-sweep backward."""
    from stablekeypoints_amd import routes
    new, old, noted = _point_loss_case(ops, routes, sides=(16, 16, 16, 32), H=8, d=40, R=128, T=77, K=10, B=2, sigma=2.0, seed=5)
    print(f"MapPointLossFn SD shapes: E error {new[0]:.2e} (older route {old[0]:.2e}), dq error {new[1]:.2e} (older route {old[1]:.2e})")
    assert noted.get(("map.bwd", "map_col")) == 1 and noted.get(("map.fwd", "map_fused")) == 1, noted
    assert new[0] <= 4 * old[0] and new[1] <= 4 * old[1], (new, old)


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. the latent gradient end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees():
    from stablekeypoints_amd.optimize_token import load_ldm
    gpu, _, _ = load_ldm("cuda", "tiny", feature_upsample_res=C.R, decoder=True)
    host, _ = C.host64()
    return gpu, host


def _older_route_grad(model, latents, context, t, pos, doubled):
    """g of the same energy through the route the package had before, inside the same fused UNet: the hooked records of the
    forward, `fused_maps` under autograd, a gather, torch ops for the target and the MSE."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd._maps import FusedAttn, fused_maps
    from stablekeypoints_amd.optimize_token import gaussian_circle
    n = pos.shape[0]
    records = []
    with torch.enable_grad():
        x = latents.detach().requires_grad_()
        ptp_utils._predict(model, x, context, t, doubled, records)
        recs = [FusedAttn(r.q[-n:], r.k if r.k.shape[0] == 1 else r.k[-n:], r.heads, r.scale, r.R) for r in records]
        M = fused_maps(recs)[:, torch.tensor(C.TOKENS, device=x.device)]
        tg = torch.stack([gaussian_circle(pos[b].to(x.device), size=C.R, sigma=C.SIGMA) for b in range(n)])
        g, = torch.autograd.grad(((M - tg) ** 2).mean(dim=(1, 2, 3)).sum(), x)
    return g[n:] if doubled else g


@pytest.mark.parametrize("case", ["plain", "guided doubled", "unequal contexts"])
def test_latent_gradient_vs_fp64(trees, case):
    """`keypoint_energy_grad` on the fused tree against the same function on the fp64 host copy, at the second timestep of the
    4-step table, n = 2: max |delta g| / max |g| within 4x the figure of the older route inside the same fused UNet, E within 1e-4
    relative, the predictions as close as the forward is."""
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    gpu, host = trees
    emb, lat, kp = C.inputs()
    gen = torch.Generator().manual_seed(41)
    uncond = {"plain": None, "guided doubled": torch.randn(1, 16, 768, generator=gen), "unequal contexts": torch.randn(1, 24, 768, generator=gen)}[case]
    doubled = case == "guided doubled"
    t = SamplerPlan(host.scheduler, "ddim", 0.0).plan(C.STEPS)[0][1]
    pc64, pu64, E64, g64 = ptp_utils.keypoint_energy_grad(host, lat.double(), [None if uncond is None else uncond.double(), emb.double()], t,
                                                          kp, list(C.TOKENS), C.SIGMA)
    ctx = [None if uncond is None else uncond.cuda(), emb.cuda()]
    x = torch.cat([lat, lat]).cuda() if doubled else lat.cuda()
    before = routes.snapshot()
    pc, pu, E, g = ptp_utils.keypoint_energy_grad(gpu, x, ctx, t, kp, list(C.TOKENS), C.SIGMA, doubled=doubled)
    noted = routes.delta(before)
    assert gpu.unet.__dict__["_skp_hook_controller"].step_store["attn"] == [] and g.shape == lat.shape and E.shape == (2,)
    assert noted.get(("sample.keypoints", "map_point_loss")) == 1 and noted.get(("conv_in.bwd_data", "small_out"), 0) >= 1, noted
    g_old = _older_route_grad(gpu, x, ctx, t, kp, doubled)
    e_new, e_old = _rel(g, g64), _rel(g_old, g64)
    print(f"latent gradient [{case}]: fused node {e_new:.2e}, older route {e_old:.2e} of max |g| = {g64.abs().max().item():.3e}; "
          f"E error {_rel(E, E64):.2e}, prediction error {_rel(pc, pc64):.2e}")
    assert (pu is None) == (uncond is None) and _rel(pc, pc64) <= 1e-4 and (pu is None or _rel(pu, pu64) <= 1e-4)
    assert ((E.double().cpu() - E64).abs() / E64).max().item() <= 1e-4
    assert e_new <= 4 * e_old, (e_new, e_old)


def test_conv_in_input_gradient(ops):
    """The input gradient of the UNet's conv_in when the latent takes one (the small-output kernel on the flipped, transposed filter)
    against torch.nn.functional.conv2d's on the same tensors in fp64: per element within the rounding bound of an fp32 sum of
    9 * Cout products, (9 Cout + 1) * 2^-24 * sum |dy| |w| (the products and the running sums, fused or not)."""
    import torch.nn.functional as F
    from stablekeypoints_amd import routes
    gen = torch.Generator().manual_seed(17)
    for B, ci, co, H, W in ((2, 4, 32, 16, 16), (1, 4, 320, 10, 6), (3, 3, 48, 5, 8)):
        x = torch.randn(B, ci, H, W, generator=gen)
        w = torch.randn(co, ci, 3, 3, generator=gen) / 3
        bias = torch.randn(co, generator=gen)
        dy = torch.randn(B, co, H, W, generator=gen)
        x64 = x.double().requires_grad_()
        y64 = F.conv2d(x64, w.double(), bias.double(), padding=1)
        dx64, = torch.autograd.grad(y64, x64, dy.double())
        mag = F.conv_transpose2d(dy.double().abs(), w.double().abs(), padding=1)
        xg, wg = x.cuda().requires_grad_(), torch.nn.Parameter(w.cuda(), requires_grad=False)
        assert ops.conv_in_grad_ok(xg, wg)
        before = routes.snapshot()
        y = ops.conv3x3_auto(xg, wg, bias.cuda())
        dx, = torch.autograd.grad(y, xg, dy.cuda())
        noted = routes.delta(before)
        assert noted == {("conv_in", "small"): 1, ("conv_in.bwd_data", "small_out"): 1}, noted
        assert _rel(y, y64.detach()) <= 1e-5
        units = ((dx.cpu().double() - dx64).abs() / (EPS * mag)).max().item()
        print(f"conv_in input gradient {ci} <- {co} at {H}x{W}: worst error {units:.2f} units of 2^-24 sum |dy||w| (bound {9 * co + 1})")
        assert units <= 9 * co + 1
    # an input that needs no gradient takes the forward kernel alone; a gradient shape the gate refuses stays on the library
    before = routes.snapshot()
    ops.conv3x3_auto(x.cuda(), wg, None)
    w40 = torch.nn.Parameter(torch.randn(40, 4, 3, 3, generator=gen).cuda(), requires_grad=False)
    x4 = torch.randn(1, 4, 8, 8, generator=gen).cuda().requires_grad_()
    assert not ops.conv_in_grad_ok(x4, w40)
    torch.autograd.grad(ops.conv3x3_auto(x4, w40).sum(), x4)
    assert routes.delta(before) == {("conv_in", "small"): 1, ("conv3x3", "lib"): 1}


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the whole call
# ---------------------------------------------------------------------------------------------------------------------------------
class _Keep:
    """A controller that keeps the latents of the last step."""
    last = None

    def step_callback(self, x):
        self.last = x
        return x

    def reset(self):
        pass


def _sample(model, scale, trace, **kw):
    from stablekeypoints_amd import ptp_utils
    emb, lat, kp = C.inputs()
    keep = _Keep()
    img, _ = ptp_utils.text2image_ldm_stable(model, emb, keep, num_inference_steps=C.STEPS, latent=lat, height=128, width=128,
                                             output_type="float", keypoints=kp, keypoint_indices=torch.tensor(C.TOKENS),
                                             keypoint_scale=scale, keypoint_sigma=C.SIGMA, keypoint_trace=trace, **kw)
    return img, keep.last


def _final(model, lat, uncond=None):
    """(E, arg-max distance) on the final latents at the last timestep of the table."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    emb, _, kp = C.inputs()
    t = SamplerPlan(model.scheduler, "ddim", 0.0).plan(C.STEPS)[0][-1]
    ctx = [uncond, emb.to(lat.device)]
    E = ptp_utils.keypoint_energy_grad(model, lat, ctx, t, kp, list(C.TOKENS), C.SIGMA)[2]
    return E.double().cpu(), C.argmax_distance(model, lat, ctx, t, kp)


def test_whole_call_vs_fp64_host_loop(trees, tune):
    """The inputs of tests/_keypoint_cases.py through `text2image_ldm_stable(keypoints=...)`, 4 steps at 128^2: the traced energies
    within 1e-3 relative of the fp64 host loop's at every step, the final energies fall by at least half of what the fp64 loop's
    fall, the mean arg-max distance is at most the fp64 loop's + 2 / R.  (No image-level tolerance: tests/test_generate_guided_gpu.py
    records that the whole-loop error gain of this seeded tree has nothing to hold one against.)"""
    from stablekeypoints_amd import routes
    gpu, _ = trees
    _, runs = C.host64()
    tune("conv_up2", 1)
    routes.reset()
    trace, trace0 = [], []
    img, lat = _sample(gpu, C.SCALE, trace)
    table = routes.table()
    snap = routes.snapshot()
    img0, lat0 = _sample(gpu, 0.0, trace0)
    assert img.shape == (2, 3, 128, 128) and img.is_cuda and len(trace) == len(trace0) == C.STEPS
    print(table)
    assert snap.get(("sample.keypoints", "map_point_loss")) == C.STEPS and snap.get(("sample.step", "sampler_step")) == C.STEPS
    assert "sample.keypoints" in table and "map_point_loss" in table and "sampler_step" in table
    assert not any(k[1] == "host" for k in snap)
    for scale, tr in ((C.SCALE, trace), (0.0, trace0)):
        for i, (e, e64) in enumerate(zip(tr, runs[scale][1])):
            err = ((e.double().cpu() - e64).abs() / e64).max().item()
            print(f"scale {scale} step {i}: E {e.tolist()} fp64 {e64.tolist()} relative error {err:.2e}")
            assert err <= 1e-3
    (E, dist), (E0, dist0) = _final(gpu, lat), _final(gpu, lat0)
    E64, d64, E064 = runs[C.SCALE][2], runs[C.SCALE][3], runs[0.0][2]
    print(f"final energy guided {E.tolist()} unguided {E0.tolist()} (fp64 {E64.tolist()} / {E064.tolist()}); distance {dist.tolist()} "
          f"(fp64 {d64.tolist()}, unguided {dist0.tolist()})")
    assert ((E0 - E) >= 0.5 * (E064 - E64)).all()
    assert (dist <= d64 + 2.0 / C.R).all()
    # two identical calls: the same bits where every backward kernel on the route sums in a fixed order, 1e-6 relative otherwise
    trace2 = []
    img2, lat2 = _sample(gpu, C.SCALE, trace2)
    same = torch.equal(img, img2) and all(torch.equal(a, b) for a, b in zip(trace, trace2))
    print("two identical calls:", "the same bits" if same else f"differ by {_rel(img2, img.double().cpu()):.2e} of the image's maximum")
    assert _rel(img2, img.double().cpu()) <= 1e-6 and _rel(lat2, lat.double().cpu()) <= 1e-6
    assert same and torch.equal(lat, lat2)                      # the bitwise case holds, and DESIGN.md says so


@pytest.mark.parametrize("sampler,prediction", [("dpm++2m", "epsilon"), (None, "v_prediction"), ("ddim", "sample")])
def test_other_samplers_and_prediction_types_run_and_lower_the_energy(tune, sampler, prediction):
    """A DPM-Solver++(2M) call, a v-prediction call and a sample-prediction call, guided by an unconditional embedding of equal
    length (the doubled loop): the energy on the final latents is below the unguided call's for every image."""
    from stablekeypoints_amd.optimize_token import load_ldm
    model, _, _ = load_ldm("cuda", "tiny", feature_upsample_res=C.R, decoder=True, prediction_type=prediction)
    tune("conv_up2", 1)
    uncond = torch.randn(1, 16, 768, generator=torch.Generator().manual_seed(41))
    kw = dict(sampler=sampler, uncond_embedding=uncond, guidance_scale=2.0, eta=0.5 if sampler == "ddim" else 0.0,
              generator=[torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)] if sampler == "ddim" else None)
    trace, trace0 = [], []
    _, lat = _sample(model, C.SCALE, trace, **kw)
    if sampler == "ddim":
        kw["generator"] = [torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)]
    _, lat0 = _sample(model, 0.0, trace0, **kw)
    (E, _), (E0, _) = _final(model, lat, uncond.cuda()), _final(model, lat0, uncond.cuda())
    print(f"{sampler} {prediction}: final energy guided {E.tolist()} unguided {E0.tolist()}")
    assert len(trace) == C.STEPS and torch.equal(trace[0], trace0[0]) and (E < E0).all()
