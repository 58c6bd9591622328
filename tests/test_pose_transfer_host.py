"""CPU tests of pose transfer (`text2image_ldm_stable(target_maps=...)`, `ptp_utils.pose_targets`): the C entries against their
header, the two energies in fp64 torch against the numpy restatement of tests/_pose_cases.py and against finite differences, the
several-points targets against the point form, the refusals of the new arguments, and the call on the reduced-width tree."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _keypoint_cases as KC
import _pose_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exports
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_and_typed():
    """include/skp_targets.h against `_native.TARGET_SIGNATURES` with the comparison tests/test_host_logic.py applies to skp.h; the
    table is disjoint from the five others; the library exports the entries, the ABI version moved, bad arguments are refused
    before any launch."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    spec = importlib.util.spec_from_file_location("_host_logic", os.path.join(ROOT, "tests", "test_host_logic.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    hdr = open(os.path.join(ROOT, "include", "skp_targets.h")).read()
    abi = H._header_abi(hdr)
    assert sorted(abi) == sorted(N.TARGET_SIGNATURES) == ["skp_map_target_loss_f32", "skp_map_target_loss_workspace"]
    assert H._abi_mismatches(hdr, N.TARGET_SIGNATURES) == []
    others = (set(N.SIGNATURES) | set(N.KEYPOINT_SIGNATURES) | set(N.OVERLAY_SIGNATURES) | set(N.LOCATE_SIGNATURES)
              | set(N.SAMPLER_GRAPH_SIGNATURES))
    assert not set(N.TARGET_SIGNATURES) & others
    assert abi["skp_map_target_loss_f32"][1][-1] == "dev:void"
    assert N.signature("skp_map_target_loss_f32") is N.TARGET_SIGNATURES["skp_map_target_loss_f32"]
    lib = N.lib()
    assert lib.skp_abi_version() == N.ABI_VERSION >= 49
    for name, argtypes in N.TARGET_SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes
    assert len(ops._plan("skp_map_target_loss_f32")[1]) == len(N.TARGET_SIGNATURES["skp_map_target_loss_f32"]) - 1
    ws = lib.skp_map_target_loss_workspace
    assert ws(2, 10, 40, 0) == 0 and ws(2, 10, 40, 1) == 24 * 2 * 10 * 2 and ws(1, 1, 1, 1) == 24
    assert ws(0, 1, 8, 1) == -1 and ws(1, 1, 8, 2) == -1 and ws(1, 1, 40000, 1) == -2 and ws(64, 32, 32768, 1) == -2 and ws(64, 31, 32768, 1) > 0
    one = 16                                                    # any non-null address: arguments are refused before a launch
    f = lib.skp_map_target_loss_f32
    assert f(None, one, 1, 1, 1, 8, 0, one, one, None, None) == -1
    assert f(one, None, 1, 1, 1, 8, 0, one, one, None, None) == -1
    assert f(one, one, 1, 1, 0, 8, 0, one, one, None, None) == -1
    assert f(one, one, 1, 1, 1, 0, 0, one, one, None, None) == -1
    assert f(one, one, 3, 2, 1, 8, 0, one, one, None, None) == -1          # two rows of targets for three images
    assert f(one, one, 1, 1, 1, 8, 2, one, one, one, None) == -1           # an unknown mode
    assert f(one, one, 1, 1, 1, 8, 1, one, one, None, None) == -1          # the cosine form needs its scratch
    assert f(one, one, 1, 1, 1, 40000, 0, one, one, None, None) == -2
    mk = open(os.path.join(ROOT, "stablekeypoints_amd", "csrc", "Makefile")).read()
    assert "skp_target_loss.hip" in mk and "skp_targets.h" in mk
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.map_target_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), "mse")
    with pytest.raises(ValueError):
        ops.map_target_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), "l1")


def test_routes_are_registered():
    from stablekeypoints_amd import routes
    assert routes.ROUTES["sample.pose"] == {"map_target_loss": "hip", "host": "host"}


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. definitions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("Bt", [1, 2])
def test_formulas_fp64_against_numpy_and_finite_differences(mode, Bt):
    """`map_target_energy` in fp64 and its autograd gradient against the numpy restatement (<= 1e-12 of the magnitudes) for every
    kind of pair, and the restated G against central differences of the restated E (step 1e-6, <= 1e-7 of max |G|)."""
    from stablekeypoints_amd.ptp_utils import map_target_energy
    B, K, R = 2, 3, 6
    for kind in C.KINDS:
        gen = torch.Generator().manual_seed(5)
        M, T = (v.double() for v in C.pair(kind, B, Bt, K, R, 1.0 / 7, gen))
        E_np, G_np, Gm, Em = C.energy_and_grad_np(M.numpy(), T.numpy(), mode)
        leaf = M.clone().requires_grad_()
        E = map_target_energy(leaf, T, mode)
        G, = torch.autograd.grad(E.sum(), leaf)
        assert np.abs(E.detach().numpy() - E_np).max() <= 1e-12 * Em.max(), kind
        assert (np.abs(G.numpy() - G_np) <= 1e-12 * Gm.max()).all(), kind
        if kind == "equal" and mode == "cosine" and Bt == B:
            assert np.abs(E_np).max() <= 1e-15 and np.abs(G_np).max() <= 1e-13        # formed from differences: nothing cancels
        if kind == "orthogonal" and mode == "cosine":
            assert np.abs(E_np - 1.0).max() <= 1e-14
        if kind == "zero map" and mode == "cosine":             # a map of zeros counts E_k = 1 and takes no gradient
            assert (G_np[:, 0] == 0).all() and (G.numpy()[:, 0] == 0).all() and np.isfinite(G.numpy()).all()
            rest = C.energy_and_grad_np(M.numpy()[:, 1:], T.numpy()[:, 1:], mode)[0]
            assert np.abs(E_np - (1.0 + (K - 1) * rest) / K).max() <= 1e-14
        if kind == "zero target" and mode == "cosine":
            assert (G_np[:, -1] == 0).all() and (G.numpy()[:, -1] == 0).all()
        if kind == "zero map" and mode == "cosine":
            continue                                            # (E is not differentiable at a map of zeros: no differences there)
        h, rng = 1e-6, np.random.default_rng(3)
        Mn = M.numpy()
        for _ in range(12):
            i = tuple(int(rng.integers(0, s)) for s in Mn.shape)
            up, dn = Mn.copy(), Mn.copy()
            up[i] += h
            dn[i] -= h
            fd = (C.energy_and_grad_np(up, T.numpy(), mode)[0][i[0]] - C.energy_and_grad_np(dn, T.numpy(), mode)[0][i[0]]) / (2 * h)
            assert abs(fd - G_np[i]) <= 1e-7 * np.abs(G_np).max() + 1e-10, (kind, i, fd, G_np[i])


def test_cosine_does_not_see_the_scale_of_either_map():
    from stablekeypoints_amd.ptp_utils import map_target_energy
    M, T = (v.double() for v in C.pair("random", 2, 2, 3, 8, 1.0, torch.Generator().manual_seed(2)))
    E = map_target_energy(M, T, "cosine")
    assert (map_target_energy(M * 77.0, T / 13.0, "cosine") - E).abs().max().item() <= 1e-14
    assert (map_target_energy(M, T[:1], "cosine") - map_target_energy(M, T[:1].expand(2, -1, -1, -1), "cosine")).abs().max().item() == 0


def test_gaussian_target_maps_with_one_point_is_the_point_form():
    """`gaussian_target_maps` with P = 1 under "mse": the energy and gradient of the point form (`find_gaussian_loss_at_point` and
    `gaussian_circle` through tests/_keypoint_cases.py) in fp64, <= 1e-12; several points combine by max / sum / mean."""
    from stablekeypoints_amd.ptp_utils import gaussian_target_maps, map_target_energy
    gen = torch.Generator().manual_seed(8)
    B, K, R = 2, 3, 8
    M = torch.rand(B, K, R, R, generator=gen, dtype=torch.float64) / 4
    pos = torch.tensor([[[.4375, .1875], [-.25, .5], [.9, 1.125]], [[.3, .71], [0., 1.], [.5, .5]]], dtype=torch.float64)
    for sigma in (0.5, 2.0):
        E_ref, G_ref, t = KC.energy_and_grad(M, pos, sigma)
        T = torch.stack([gaussian_target_maps(pos[b][:, None], R, sigma) for b in range(B)])
        assert T.shape == (B, K, R, R) and (T - t).abs().max().item() <= 1e-12
        leaf = M.clone().requires_grad_()
        E = map_target_energy(leaf, T, "mse")
        G, = torch.autograd.grad(E.sum(), leaf)
        assert (E.detach() - E_ref).abs().max().item() <= 1e-12 and (G - G_ref).abs().max().item() <= 1e-12
        E_np, G_np, _, _ = C.energy_and_grad_np(M.numpy(), T.numpy(), "mse")
        assert np.abs(E_np - E_ref.numpy()).max() <= 1e-12 and np.abs(G_np - G_ref.numpy()).max() <= 1e-12
    pts = torch.tensor([[[.25, .25], [.75, .75]], [[.5, .1], [.5, .9]]], dtype=torch.float64)             # K = 2, P = 2
    each = torch.stack([gaussian_target_maps(pts[:, p:p + 1], R, 1.0) for p in range(2)])
    assert torch.equal(gaussian_target_maps(pts, R, 1.0), each.amax(dim=0))
    assert (gaussian_target_maps(pts, R, 1.0, reduce="sum") - each.sum(dim=0)).abs().max().item() <= 1e-15
    assert (gaussian_target_maps(pts, R, 1.0, reduce="mean") - each.mean(dim=0)).abs().max().item() <= 1e-15
    for bad in (dict(points=pts[0]), dict(points=pts, reduce="min"), dict(points=pts[..., :1])):
        with pytest.raises(ValueError):
            gaussian_target_maps(**{"points": pts, "R": R, "sigma": 1.0, **bad})


def test_the_resample_is_the_identity_at_the_models_resolution():
    from stablekeypoints_amd.ptp_utils import resample_target_maps
    T = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    assert resample_target_maps(T, 32) is T
    down = resample_target_maps(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)), 32)
    assert down.shape == (1, 3, 32, 32)
    flat = resample_target_maps(torch.full((1, 2, 48, 48), 0.25), 32)          # a constant stays the constant
    assert (flat - 0.25).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the call (float32 modules on the host route)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from stablekeypoints_amd.optimize_token import load_ldm
    model, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=KC.R, decoder=True)
    return model, next(iter(controllers.values()))


@pytest.fixture(scope="module")
def targets(tiny):
    return C.example_targets(tiny[0])


def _call(tiny, **kw):
    from stablekeypoints_amd import ptp_utils
    model, controller = tiny
    emb, lat, _ = KC.inputs()
    kw.setdefault("latent", lat[:, :, :8, :8].contiguous())
    return ptp_utils.text2image_ldm_stable(model, emb, controller, num_inference_steps=2, height=64, width=64, output_type="float", **kw)


def test_pose_targets(tiny, targets):
    """[1, K, R, R], the quantity the energy reads: the maps `collect_maps_batched` semantics give for the K tokens (the host
    formula: a softmax over the 16 tokens, so every pixel of a map lies in (0, 1)); the store is empty afterwards; two images give
    two rows, the first the single call's."""
    from stablekeypoints_amd import ptp_utils
    model, controller = tiny
    assert targets.shape == (1, len(KC.TOKENS), KC.R, KC.R) and targets.dtype == torch.float32
    assert bool((targets > 0).all()) and bool((targets < 1).all())
    assert controller.step_store["attn"] == [] and model.unet.__dict__["_skp_hook_controller"].step_store["attn"] == []
    emb, _, _ = KC.inputs()
    img = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(4))
    noise = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(5))
    both = ptp_utils.pose_targets(model, img, emb, list(KC.TOKENS), noise=noise)
    one = ptp_utils.pose_targets(model, img[0], emb, torch.tensor(KC.TOKENS), noise=noise[:1])
    assert both.shape == (2, 3, KC.R, KC.R) and (both[:1] - one).abs().max().item() <= 1e-6
    for bad in ([2, 2, 7], [2, 7, 16], []):
        with pytest.raises(ValueError):
            ptp_utils.pose_targets(model, img, emb, bad, noise=noise)


def test_every_value_error_of_the_new_arguments(tiny, targets):
    ids = torch.tensor(KC.TOKENS)
    kp = torch.tensor(KC.TARGETS)
    for bad in (dict(target_maps=targets),                                                         # maps without token ids
                dict(target_maps=targets, keypoint_indices=ids, keypoints=kp),                     # both kinds of target
                dict(target_maps=targets[:, :2], keypoint_indices=ids),                            # a wrong K
                dict(target_maps=targets.expand(3, -1, -1, -1), keypoint_indices=ids),             # three rows for two images
                dict(target_maps=targets[..., :31], keypoint_indices=ids),                         # not square
                dict(target_maps=targets[0, 0], keypoint_indices=ids),                             # not [K, R, R]
                dict(target_maps=targets, keypoint_indices=ids, target_energy="l1"),
                dict(target_maps=targets, keypoint_indices=[2, 7, 7]),
                dict(target_maps=targets, keypoint_indices=[2, 7, 16])):
        with pytest.raises(ValueError):
            _call(tiny, **bad)
    gen = torch.Generator().manual_seed(1)                      # a bad argument fails before anything is drawn from the generator
    state = gen.get_state()
    for bad in (dict(target_maps=targets[:, :2], keypoint_indices=ids), dict(target_maps=targets.expand(2, -1, -1, -1), keypoint_indices=ids),
                dict(target_maps=targets, keypoint_indices=ids, target_energy="l2"), dict(target_maps=targets[..., :31], keypoint_indices=ids)):
        with pytest.raises(ValueError):
            _call(tiny, latent=None, generator=gen, **bad)
    assert torch.equal(gen.get_state(), state)
    from stablekeypoints_amd import ptp_utils
    emb, lat, _ = KC.inputs()
    with pytest.raises(ValueError):
        ptp_utils.keypoint_energy_grad(tiny[0], lat, [None, emb], torch.tensor(500), kp, list(KC.TOKENS), 2.0, target_maps=targets)


def test_call_hygiene_and_shapes_of_targets(tiny, targets):
    """[K, R, R], [1, K, R, R] and n equal rows are one call; targets at 2R are resampled; the trace, the scheduler, the store and
    the parameters are left as the point form leaves them; an empty window is the unguided plan call; the ledger names the host."""
    from stablekeypoints_amd import routes
    model, controller = tiny
    ids = torch.tensor(KC.TOKENS)
    table = (model.scheduler.timesteps, model.scheduler.num_inference_steps)
    trace = []
    before = routes.snapshot()
    img, _ = _call(tiny, target_maps=targets, keypoint_indices=ids, keypoint_trace=trace)
    noted = routes.delta(before)
    assert noted.get(("sample.pose", "host")) == 2 and ("sample.keypoints", "host") not in noted
    assert img.shape == (2, 3, 64, 64) and len(trace) == 2 and all(e.shape == (2,) for e in trace)
    assert model.scheduler.timesteps is table[0] and model.scheduler.num_inference_steps == table[1]
    assert controller.step_store["attn"] == [] and model.unet.__dict__["_skp_hook_controller"].step_store["attn"] == []
    assert not any(p.grad is not None for p in model.unet.parameters())
    a, _ = _call(tiny, target_maps=targets[0], keypoint_indices=ids)
    b, _ = _call(tiny, target_maps=targets.expand(2, -1, -1, -1), keypoint_indices=ids)
    assert torch.equal(a, img) and torch.equal(b, img)
    mse, _ = _call(tiny, target_maps=targets, keypoint_indices=ids, target_energy="mse")
    plain, _ = _call(tiny, sampler="ddim")
    off, _ = _call(tiny, target_maps=targets, keypoint_indices=ids, keypoint_steps=(0, 0))
    assert not torch.equal(mse, img) and not torch.equal(img, plain) and (off - plain).abs().max().item() <= 1e-5
    big = torch.nn.functional.interpolate(targets, size=(64, 64), mode="bilinear", align_corners=False)
    up, _ = _call(tiny, target_maps=big, keypoint_indices=ids)
    assert up.shape == img.shape and bool(torch.isfinite(up).all()) and not torch.equal(up, plain)


@pytest.mark.parametrize("mode", C.MODES)
def test_host_fp64_loop_lowers_the_energy(targets, mode):
    """The fp64 host loop on the reduced-width tree, 4 steps at 128^2 with the example's maps as targets: the traced energy falls
    from the first guided step to the last for every image, and the final energy is below the unguided loop's."""
    runs = C.host64_runs(targets)
    _, trace, E = runs[(mode, KC.SCALE)]
    _, trace0, E0 = runs[(mode, 0.0)]
    print(mode, "trace", [e.tolist() for e in trace], "final", E.tolist(), "unguided", E0.tolist())
    assert len(trace) == len(trace0) == KC.STEPS and torch.equal(trace[0], trace0[0])
    assert (trace[-1] < trace[0]).all() and (E < E0).all()


def test_the_call_with_targets_shows_the_energy_falling(tiny, targets):
    """`text2image_ldm_stable(target_maps=...)` itself (float32 modules on the host route), 4 steps at 128^2: `keypoint_trace` falls."""
    from stablekeypoints_amd import ptp_utils
    model, controller = tiny
    emb, lat, _ = KC.inputs()
    trace = []
    ptp_utils.text2image_ldm_stable(model, emb, controller, num_inference_steps=KC.STEPS, latent=lat, height=128, width=128,
                                    output_type="float", target_maps=targets, keypoint_indices=torch.tensor(KC.TOKENS), keypoint_trace=trace)
    assert len(trace) == KC.STEPS and (trace[-1] < trace[0]).all()
    want = C.host64_runs(targets)[("cosine", KC.SCALE)][1]
    assert max(((a.double() - b).abs() / b).max().item() for a, b in zip(trace, want)) <= 1e-2      # the loop the fp64 copy writes out


def test_without_targets_the_call_is_what_it_was(tiny):
    """With `target_maps=None` (passed by name) the loop of the call as it was, written out on the scheduler's own step, gives the
    same bytes, and the point form's call notes its own site alone."""
    from stablekeypoints_amd import ptp_utils, routes
    model, _ = tiny
    emb, lat, _ = KC.inputs()
    lat = lat[:, :, :8, :8].contiguous()
    img, _ = _call(tiny, target_maps=None, target_energy="cosine")
    with torch.no_grad():
        kept = (model.scheduler.timesteps, model.scheduler.num_inference_steps)
        model.scheduler.set_timesteps(2)
        x = lat
        for t in model.scheduler.timesteps:
            x = model.scheduler.step(ptp_utils.diffusion_step(model, x, emb, t), t, x)["prev_sample"]
        model.scheduler.timesteps, model.scheduler.num_inference_steps = kept
        assert torch.equal(img, ptp_utils._latent2float(model.vae, x))
    before = routes.snapshot()
    _call(tiny, keypoints=torch.tensor(KC.TARGETS), keypoint_indices=torch.tensor(KC.TOKENS), target_maps=None)
    noted = routes.delta(before)
    assert noted.get(("sample.keypoints", "host")) == 2 and not any(k[0] == "sample.pose" for k in noted)
