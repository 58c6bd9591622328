"""Pose transfer on the MI355X: the target-loss kernel against fp64 with counted per-element bounds, `ops.MapTargetLossFn` and
`ptp_utils.keypoint_energy_grad(target_maps=...)` against the fp64 host formula (held to the bands of the point form's tests, which
run alongside as the yardstick), `text2image_ldm_stable(target_maps=...)` against the fp64 host loop of tests/_pose_cases.py, and the
captured loop against the eager one bit for bit.  The measured figures are recorded in profiles/generate_pose.md."""
import itertools

import numpy as np
import pytest
import torch

import _keypoint_cases as KC
import _pose_cases as C

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
# 1. the target-loss kernel
# ---------------------------------------------------------------------------------------------------------------------------------
# Roundings into G, in units of 2^-24 of the magnitude of its formula (mse: 2 (|M| + |T|) / (K R^2); cosine: (|mh| + |th|) / (K sqrt(a))).
# Everything between the float inputs and the float G is fp64: the products M M, T T, M T and M - T are exact there, the 1024-element
# and per-map sums, the square roots, quotients and the few products per element each carry 2^-53, together under 2^-40 of the
# magnitude.  That leaves the one conversion of G to a float: 1 unit.  Rounded up to 2.
U_G = 2.0
# The energy, in units of 2^-24 of mean (|M| + |T|)^2 (mse) or of (1/K) sum_k 1/2 sum (|mh| + |th|)^2 (cosine; a map of zeros counts its
# E_k = 1): each chunk sum is formed in fp64 and converted to a float once, 1; the sum of the K * nchunk chunk sums (at most 528
# here) in torch's reduction tree at most 16 more, as counted for the point form; the division by K R^2 or 2 K 1: 18.
U_E = 18.0


@pytest.mark.parametrize("B,K,R", [(1, 1, 16), (3, 3, 32), (2, 10, 40), (1, 33, 128)])
def test_map_target_loss_vs_fp64(ops, B, K, R):
    """R^2 below, equal to and ragged against the 1024-element chunk and of many chunks, K beyond 32; both modes; a target per
    image and one shared; maps of softmax scale and of unit scale; targets that are random, equal to the map (where 1 - cos
    cancels), orthogonal to it, and a map or a target of zeros among the K.  Per element |G - G64| <= 2 * 2^-24 of the magnitude of
    G's formula, |E - E64| <= 18 * 2^-24 of the magnitude of E's; G is exactly 0 where that magnitude is; two calls give the same
    bits."""
    gen = torch.Generator().manual_seed(200 + R)
    worst_g = worst_e = 0.0
    for mode, Bt, scale, kind in itertools.product(C.MODES, sorted({1, B}), (1.0 / 77, 1.0), C.KINDS):
        M, T = C.pair(kind, B, Bt, K, R, scale, gen)
        Mg, Tg = M.cuda(), T.cuda()
        E, G = ops.map_target_loss(Mg, Tg, mode)
        E2, G2 = ops.map_target_loss(Mg, Tg, mode)
        where = (mode, Bt, scale, kind)
        assert torch.equal(E, E2) and torch.equal(G, G2) and E.shape == (B,) and G.shape == M.shape, where
        assert torch.equal(Mg.cpu(), M) and torch.equal(Tg.cpu(), T)                     # the inputs are only read
        E64, G64, Gm, Em = C.energy_and_grad_np(M.numpy(), T.numpy(), mode)
        eg = np.abs(G.cpu().double().numpy() - G64)
        assert (eg[Gm == 0] == 0).all(), where
        ug = float((eg[Gm > 0] / (EPS * Gm[Gm > 0])).max()) if (Gm > 0).any() else 0.0
        ue = float((np.abs(E.cpu().double().numpy() - E64) / (EPS * Em)).max())
        worst_g, worst_e = max(worst_g, ug), max(worst_e, ue)
        assert ug <= U_G and ue <= U_E, (where, ug, ue)
        if mode == "cosine" and kind == "equal" and Bt == B:
            assert bool((E == 0).all())                                                 # formed from the differences: exact zeros
        if mode == "cosine" and kind == "zero map":
            assert bool((G[:, 0] == 0).all()) and bool(torch.isfinite(G).all()) and bool(torch.isfinite(E).all())
            if K == 1:
                assert bool((E == 1).all())
    print(f"map_target_loss B={B} K={K} R={R}: worst G error {worst_g:.2f} units (bound {U_G:.0f}), worst E error {worst_e:.2f} units "
          f"(bound {U_E:.0f})")


def test_map_target_loss_refuses_wrong_shapes(ops):
    M = torch.zeros(2, 3, 8, 8, device="cuda")
    for bad in (torch.zeros(3, 3, 8, 8), torch.zeros(2, 2, 8, 8), torch.zeros(2, 3, 8, 4), torch.zeros(3, 8, 8)):
        with pytest.raises(RuntimeError):
            ops.map_target_loss(M, bad.cuda(), "mse")
    with pytest.raises(RuntimeError):
        ops.map_target_loss(M, torch.zeros(2, 3, 8, 8, device="cuda", dtype=torch.float64), "cosine")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. MapTargetLossFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _target_loss_case(ops, routes, mode, Bt, sides, H, d, R, T, K, B, sigma, seed):
    """-> ((E error, dq error) of MapTargetLossFn, the same of the older route, routes noted by the first), errors as max |delta| /
    max |ref| against the fp64 host formula on the same q / k (those of `_point_loss_case` for this seed) and random targets of
    softmax scale."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd._maps import FusedAttn, _materialize_host, fused_maps
    gen = torch.Generator().manual_seed(seed)
    scales = [d ** -0.5] * len(sides)
    qs = [torch.randn(B, s * s, H * d, generator=gen) for s in sides]
    ks = [torch.randn(1, T, H * d, generator=gen) for _ in sides]
    ids = sorted(torch.randperm(T, generator=gen)[:K].tolist())
    target = torch.rand(Bt, K, R, R, generator=gen) * (2.0 / T)
    q64 = [q.double().requires_grad_() for q in qs]
    M64 = sum(_materialize_host(q, k.double(), H, sc, R).reshape(B, H, R * R, -1)[..., ids].mean(dim=1) for q, k, sc in zip(q64, ks, scales))
    M64 = (M64 / len(qs)).permute(0, 2, 1).reshape(B, K, R, R)
    E64 = ptp_utils.map_target_energy(M64, target.double(), mode)
    dq64 = torch.autograd.grad(E64.sum(), q64)
    E64 = E64.detach()

    def errors(E, dq):
        return _rel(E, E64), max(_rel(a, b) for a, b in zip(dq, dq64))

    qg = [q.cuda().requires_grad_() for q in qs]
    kg = [k.cuda() for k in ks]
    sel = torch.tensor(ids, device="cuda")
    tokrow = torch.full((T,), -1, dtype=torch.int32)
    tokrow[ids] = torch.arange(K, dtype=torch.int32)
    meta = dict(R=R, heads=H, scales=scales, target=target.cuda(), mode=mode, sel=sel, tokrow=tokrow.cuda())
    before = routes.snapshot()
    E = ops.MapTargetLossFn.apply(meta, *[v for q, k in zip(qg, kg) for v in (q, k)])
    dq = torch.autograd.grad(E.sum(), qg)
    noted = routes.delta(before)
    new = errors(E, dq)
    # the route the package would have had without the node: dense fused maps under autograd, a gather, the formula in torch ops
    Mo = fused_maps([FusedAttn(q, k, H, sc, R) for q, k, sc in zip(qg, kg, scales)])[:, sel]
    Eo = ptp_utils.map_target_energy(Mo, target.cuda(), mode)
    old = errors(Eo, torch.autograd.grad(Eo.sum(), qg))
    return new, old, noted


@pytest.mark.parametrize("bwd", ["auto", "sweep", "dense"])
@pytest.mark.parametrize("T", [16, 160])
def test_map_target_loss_fn_vs_fp64_tiny_shapes(ops, monkeypatch, bwd, T):
    """The shapes of test_map_point_loss_fn_vs_fp64_tiny_shapes (sides 4, 4, 4, 8; 4 heads of 16 channels; R = 32; 16 tokens and 160)
    under every map-backward mode, both energies, a target per image and one shared: E and dq within 4x the error of the older
    route on the same inputs against the same fp64 -- that test's band -- with the point form run here as the yardstick, held to
    the same band; the ledger names the same map routes for both nodes."""
    from stablekeypoints_amd import routes
    from test_keypoint_guidance_gpu import TINY, _point_loss_case
    monkeypatch.setattr(ops, "MAP_BWD_MODE", bwd)
    p_new, p_old, p_noted = _point_loss_case(ops, routes, T=T, seed=7 + T, **TINY)
    print(f"MapPointLossFn tiny T={T} mode={bwd}: E error {p_new[0]:.2e} (older route {p_old[0]:.2e}), dq error {p_new[1]:.2e} (older "
          f"route {p_old[1]:.2e})")
    assert p_new[0] <= 4 * p_old[0] and p_new[1] <= 4 * p_old[1], (p_new, p_old)
    for mode, Bt in itertools.product(C.MODES, (1, TINY["B"])):
        new, old, noted = _target_loss_case(ops, routes, mode, Bt, T=T, seed=7 + T, **TINY)
        print(f"MapTargetLossFn tiny T={T} mode={bwd} {mode} Bt={Bt}: E error {new[0]:.2e} (older route {old[0]:.2e}), dq error "
              f"{new[1]:.2e} (older route {old[1]:.2e})")
        assert {k: v for k, v in noted.items() if k[0].startswith("map.")} == {k: v for k, v in p_noted.items() if k[0].startswith("map.")}
        assert new[0] <= 4 * old[0] and new[1] <= 4 * old[1], (mode, Bt, new, old)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the latent gradient end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees():
    from stablekeypoints_amd.optimize_token import load_ldm
    gpu, _, _ = load_ldm("cuda", "tiny", feature_upsample_res=KC.R, decoder=True)
    return gpu, C.host64_model()


@pytest.fixture(scope="module")
def pose(trees):
    """`pose_targets` [1, K, R, R] on the GPU tree, of an image the same tree sampled with another seed."""
    tg = C.example_targets(trees[0])
    assert tg.shape == (1, len(KC.TOKENS), KC.R, KC.R) and tg.is_cuda and tg.dtype == torch.float32
    assert trees[0].unet.__dict__["_skp_hook_controller"].step_store["attn"] == []
    return tg


def _older_route_grad(model, latents, context, t, targets, mode, doubled):
    """g of the same energy through the route without the node, inside the same fused UNet: the hooked records of the forward,
    `fused_maps` under autograd, a gather, the formula in torch ops."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd._maps import FusedAttn, fused_maps
    n = latents.shape[0] // 2 if doubled else latents.shape[0]
    records = []
    with torch.enable_grad():
        x = latents.detach().requires_grad_()
        ptp_utils._predict(model, x, context, t, doubled, records)
        recs = [FusedAttn(r.q[-n:], r.k if r.k.shape[0] == 1 else r.k[-n:], r.heads, r.scale, r.R) for r in records]
        M = fused_maps(recs)[:, torch.tensor(KC.TOKENS, device=x.device)]
        g, = torch.autograd.grad(ptp_utils.map_target_energy(M, targets, mode).sum(), x)
    model.unet.__dict__["_skp_hook_controller"].reset()
    return g[n:] if doubled else g


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("case", ["plain", "guided doubled", "unequal contexts"])
def test_latent_gradient_vs_fp64(trees, pose, case, mode):
    """`keypoint_energy_grad(target_maps=...)` on the fused tree against the same function on the fp64 host copy, at the second
    timestep of the 4-step table, n = 2 (one shared target; a target per image in the last case): the band of the point form's
    test_latent_gradient_vs_fp64 -- max |delta g| / max |g| within 4x the figure of the older route inside the same fused UNet, E
    within 1e-4 relative, the predictions within 1e-4."""
    from stablekeypoints_amd import ptp_utils, routes
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    gpu, host = trees
    emb, lat, _ = KC.inputs()
    gen = torch.Generator().manual_seed(41)
    uncond = {"plain": None, "guided doubled": torch.randn(1, 16, 768, generator=gen), "unequal contexts": torch.randn(1, 24, 768, generator=gen)}[case]
    doubled = case == "guided doubled"
    tg = torch.cat([pose, pose.flip(1)]) if case == "unequal contexts" else pose
    kw = dict(target_energy=mode)
    t = SamplerPlan(host.scheduler, "ddim", 0.0).plan(KC.STEPS)[0][1]
    pc64, pu64, E64, g64 = ptp_utils.keypoint_energy_grad(host, lat.double(), [None if uncond is None else uncond.double(), emb.double()], t,
                                                          None, list(KC.TOKENS), None, target_maps=tg.double().cpu(), **kw)
    ctx = [None if uncond is None else uncond.cuda(), emb.cuda()]
    x = torch.cat([lat, lat]).cuda() if doubled else lat.cuda()
    before = routes.snapshot()
    pc, pu, E, g = ptp_utils.keypoint_energy_grad(gpu, x, ctx, t, None, list(KC.TOKENS), None, doubled=doubled, target_maps=tg, **kw)
    noted = routes.delta(before)
    assert gpu.unet.__dict__["_skp_hook_controller"].step_store["attn"] == [] and g.shape == lat.shape and E.shape == (2,)
    assert noted.get(("sample.pose", "map_target_loss")) == 1 and not any(k[0] == "sample.keypoints" for k in noted), noted
    assert noted.get(("conv_in.bwd_data", "small_out"), 0) >= 1, noted
    g_old = _older_route_grad(gpu, x, ctx, t, tg, mode, doubled)
    e_new, e_old = _rel(g, g64), _rel(g_old, g64)
    print(f"pose latent gradient [{case}, {mode}]: fused node {e_new:.2e}, older route {e_old:.2e} of max |g| = "
          f"{g64.abs().max().item():.3e}; E error {((E.double().cpu() - E64).abs() / E64).max().item():.2e}, prediction error "
          f"{_rel(pc, pc64):.2e}")
    assert (pu is None) == (uncond is None) and _rel(pc, pc64) <= 1e-4 and (pu is None or _rel(pu, pu64) <= 1e-4)
    assert ((E.double().cpu() - E64).abs() / E64).max().item() <= 1e-4
    assert e_new <= 4 * e_old, (e_new, e_old)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the whole call
# ---------------------------------------------------------------------------------------------------------------------------------
def _sample(model, pose, mode, scale, trace, **kw):
    from stablekeypoints_amd import ptp_utils
    from test_keypoint_guidance_gpu import _Keep
    emb, lat, _ = KC.inputs()
    keep = _Keep()
    img, _ = ptp_utils.text2image_ldm_stable(model, emb, keep, num_inference_steps=KC.STEPS, latent=lat, height=128, width=128,
                                             output_type="float", target_maps=pose, target_energy=mode,
                                             keypoint_indices=torch.tensor(KC.TOKENS), keypoint_scale=scale, keypoint_trace=trace, **kw)
    return img, keep.last


def _final(model, lat, pose, mode, uncond=None):
    """E on the final latents at the last timestep of the table."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    emb, _, _ = KC.inputs()
    t = SamplerPlan(model.scheduler, "ddim", 0.0).plan(KC.STEPS)[0][-1]
    E = ptp_utils.keypoint_energy_grad(model, lat, [uncond, emb.to(lat.device)], t, None, list(KC.TOKENS), None, target_maps=pose,
                                       target_energy=mode)[2]
    return E.double().cpu()


@pytest.mark.parametrize("mode", C.MODES)
def test_whole_call_vs_fp64_host_loop(trees, pose, tune, mode):
    """The inputs of tests/_keypoint_cases.py through `text2image_ldm_stable(target_maps=...)` with the example's maps, 4 steps at
    128^2, the band of the point form's whole-call test: the traced energies within 1e-3 relative of the fp64 host loop's at every
    step, the final energies fall by at least half of what the fp64 loop's fall -- and are below the unguided call's; the site
    `sample.pose` reads `map_target_loss` once per step and nothing ran on the host; two identical calls give the same bits."""
    from stablekeypoints_amd import routes
    gpu, _ = trees
    runs = C.host64_runs(pose.cpu())
    tune("conv_up2", 1)
    routes.reset()
    trace, trace0 = [], []
    img, lat = _sample(gpu, pose, mode, KC.SCALE, trace)
    snap = routes.snapshot()
    img0, lat0 = _sample(gpu, pose, mode, 0.0, trace0)
    assert img.shape == (2, 3, 128, 128) and img.is_cuda and len(trace) == len(trace0) == KC.STEPS
    assert snap.get(("sample.pose", "map_target_loss")) == KC.STEPS and snap.get(("sample.step", "sampler_step")) == KC.STEPS
    assert not any(k[1] == "host" for k in snap) and not any(k[0] == "sample.keypoints" for k in snap)
    for scale, tr in ((KC.SCALE, trace), (0.0, trace0)):
        for i, (e, e64) in enumerate(zip(tr, runs[(mode, scale)][1])):
            err = ((e.double().cpu() - e64).abs() / e64).max().item()
            print(f"{mode} scale {scale} step {i}: E {e.tolist()} fp64 {e64.tolist()} relative error {err:.2e}")
            assert err <= 1e-3
    E, E0 = _final(gpu, lat, pose, mode), _final(gpu, lat0, pose, mode)
    E64, E064 = runs[(mode, KC.SCALE)][2], runs[(mode, 0.0)][2]
    print(f"{mode}: final energy guided {E.tolist()} unguided {E0.tolist()} (fp64 {E64.tolist()} / {E064.tolist()})")
    assert (E < E0).all() and ((E0 - E) >= 0.5 * (E064 - E64)).all()
    trace2 = []
    img2, lat2 = _sample(gpu, pose, mode, KC.SCALE, trace2)
    assert torch.equal(img, img2) and torch.equal(lat, lat2) and all(torch.equal(a, b) for a, b in zip(trace, trace2))


def test_strict_routes_name_the_pose_site(trees, pose, tune):
    """The call under `routes.strict(allow=DOCUMENTED_LIBRARY_ROUTES)`: it passes, and the site `sample.pose` reads
    `map_target_loss` once per step.  (Inside `ops.conv3x3_own_kernels()`, as tests/test_evaluate_gpu.py runs strict: two rows of
    the reduced tree at 128^2 have too few tiles at the inner levels for `conv3x3_plan`'s tile rule, with or without targets.)"""
    from stablekeypoints_amd import ops, routes
    gpu, _ = trees
    tune("conv_up2", 1)
    routes.reset()
    trace = []
    with ops.conv3x3_own_kernels(), routes.strict(allow=routes.DOCUMENTED_LIBRARY_ROUTES):
        img, _ = _sample(gpu, pose, "cosine", KC.SCALE, trace)
    snap = routes.snapshot()
    print(routes.table())
    assert snap.get(("sample.pose", "map_target_loss")) == KC.STEPS and len(trace) == KC.STEPS and bool(torch.isfinite(img).all())
    assert all(routes.kind(s, r) == "hip" or (s, r) in routes.DOCUMENTED_LIBRARY_ROUTES for s, r in snap if snap[(s, r)])


@pytest.mark.parametrize("mode", C.MODES)
def test_another_sampler_runs_and_lowers_the_energy(trees, pose, tune, mode):
    """A DPM-Solver++(2M) call guided by an unconditional embedding of equal length (the doubled loop), a target per image: the
    energy on the final latents is below the unguided call's for every image."""
    model, _ = trees
    tune("conv_up2", 1)
    uncond = torch.randn(1, 16, 768, generator=torch.Generator().manual_seed(41))
    tg = torch.cat([pose, pose.flip(1)])
    kw = dict(sampler="dpm++2m", uncond_embedding=uncond, guidance_scale=2.0)
    trace, trace0 = [], []
    _, lat = _sample(model, tg, mode, KC.SCALE, trace, **kw)
    _, lat0 = _sample(model, tg, mode, 0.0, trace0, **kw)
    E, E0 = _final(model, lat, tg, mode, uncond.cuda()), _final(model, lat0, tg, mode, uncond.cuda())
    print(f"dpm++2m {mode}: final energy guided {E.tolist()} unguided {E0.tolist()}")
    assert len(trace) == KC.STEPS and torch.equal(trace[0], trace0[0]) and (E < E0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the captured loop
# ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_with_targets(trees, pose, tune):
    """6 steps at 128^2, two images, guided over the first half (so both graphs replay): `capture=True` with targets equals the
    eager call bit for bit in latents, image and trace; a second call with other target VALUES finds the recorded step and gives
    the bits of its own eager call; the other energy is another key."""
    from stablekeypoints_amd import ptp_utils
    from test_sample_graph_gpu import _pair
    ldm, _ = trees
    ctrl = ldm.unet.__dict__["_skp_hook_controller"]
    tune("conv_up2", 1)
    emb, lat, _ = KC.inputs()
    cache = ptp_utils.sample_graphs(ldm)
    cache.clear()
    other = (pose.flip(1) * 1.5 + 0.001).contiguous()
    results = []
    for k, (tg, mode, want) in enumerate(((pose, "cosine", "miss"), (other, "cosine", "hit"), (other, "mse", "miss"))):
        traces = []

        def make_kw():
            traces.append([])
            return dict(height=128, width=128, latent=lat, target_maps=tg, target_energy=mode, keypoint_indices=torch.tensor(KC.TOKENS),
                        keypoint_scale=KC.SCALE, keypoint_steps=(0.0, 0.5), keypoint_trace=traces[-1])
        hits, misses = cache.hits, cache.misses
        (img0, lat0), (img1, lat1), d = _pair(ldm, ctrl, emb, make_kw, 6)
        assert torch.equal(lat1, lat0), f"call {k}: final latents differ by {(lat1 - lat0).abs().max().item():.3e}"
        assert torch.equal(img1, img0), k
        assert len(traces[0]) == len(traces[1]) == 3 and all(torch.equal(a, b) for a, b in zip(*traces)), k
        assert d.get(("sample.pose", "map_target_loss")) == 3 and d.get(("sample.step", "sampler_step")) == 6, d
        assert cache.last == want and (cache.hits, cache.misses) == (hits + (want == "hit"), misses + (want == "miss")), (k, cache.last)
        assert sorted(cache.entries[cache.last_key].graphs) == ["kp", "plain"]
        assert cache.last_key[-2] == ("maps", mode, KC.R, 1, True)
        results.append(img1)
    assert len(cache.keys()) == 2 and not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
