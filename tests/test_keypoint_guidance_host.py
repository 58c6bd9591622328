"""CPU tests of keypoint guidance (`text2image_ldm_stable(keypoints=...)`): its definitions against the reference's own helpers in
fp64, the gradient term of `samplers.step_formula`, the behaviour on the fixed inputs of tests/_keypoint_cases.py, the hygiene of the
call, and the two C entries with their header."""
import importlib.util
import os

import pytest
import torch

import _keypoint_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. definitions
# ---------------------------------------------------------------------------------------------------------------------------------
def _host_energy(M, pos, sigma):
    """E of `keypoint_energy_grad`'s host branch, through a fake one-layer record whose softmax IS the given maps:
    one head, layer side R (no resize), logits log(M) with a rest token that completes every pixel's distribution."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd._maps import FusedAttn
    B, K, R, _ = M.shape
    rest = 1 - M.sum(dim=1, keepdim=True)
    assert (rest > 0).all()
    probs = torch.cat([M, rest], dim=1).reshape(B, K + 1, R * R).permute(0, 2, 1).clone().requires_grad_()   # [B, R^2, T]

    class Unet(torch.nn.Module):
        def forward(self, x, t, ctx):
            # q = log-probabilities [B, R^2, T], k = identity [1, T, T], scale 1: softmax_t(q k^T) = probs
            self._skp_hook_controller.step_store["attn"].append(FusedAttn(probs.log() + 0 * x.sum(), torch.eye(K + 1, dtype=M.dtype)[None], 1, 1.0, R))
            return {"sample": x}

    class Store:
        def __init__(self):
            self.step_store = {"attn": []}

        def reset(self):
            self.step_store = {"attn": []}

    model = type("M", (), {})()
    model.unet = Unet()
    model.unet.__dict__["_skp_hook_controller"] = Store()
    x = torch.zeros(B, 1, 2, 2, dtype=M.dtype)
    ctx = torch.zeros(1, K + 1, 4, dtype=M.dtype)
    _, _, E, g = ptp_utils.keypoint_energy_grad(model, x, [None, ctx], torch.tensor(0), pos, list(range(K)), sigma, layers=(0,))
    assert model.unet.__dict__["_skp_hook_controller"].step_store["attn"] == [] and g.shape == x.shape
    return E


@pytest.mark.parametrize("name,B,K,R,pos", [
    ("pixel centres", 2, 3, 8, [[[.4375, .1875], [.0625, .9375], [.5625, .5625]], [[.9375, .0625], [.3125, .3125], [.6875, .8125]]]),
    ("outside", 1, 2, 8, [[[-.25, .5], [1.5, 1.125]]]),
    ("K = 1", 2, 1, 6, [[[.3, .71]], [[0., 1.]]]),
])
def test_definitions_against_the_reference_helpers_fp64(name, B, K, R, pos):
    """E of the host branch against `find_gaussian_loss_at_point`, and the written-out G = 2 (M - t) / (K R^2), t the formula of
    the kernel's header, against that function's own gradient and `gaussian_circle`: <= 1e-12."""
    g = torch.Generator().manual_seed(11)
    M = torch.rand(B, K, R, R, generator=g, dtype=torch.float64) / (K + 1)
    pos = torch.tensor(pos, dtype=torch.float32)
    for sigma in (0.5, 2.0):
        E_ref, G_ref, t = C.energy_and_grad(M, pos, sigma)
        if name == "pixel centres":                            # the target's peak is a pixel, and it is 1 there
            assert torch.equal(t.reshape(B, K, -1).max(dim=-1).values, torch.ones(B, K, dtype=torch.float64))
        assert (_host_energy(M, pos, sigma) - E_ref).abs().max().item() <= 1e-12
        p, ar = pos.double() * R, torch.arange(R, dtype=torch.float64) + 0.5
        t2 = torch.exp(-((ar.view(1, 1, 1, R) - p[..., 1, None, None]) ** 2 + (ar.view(1, 1, R, 1) - p[..., 0, None, None]) ** 2)
                       / (2 * sigma ** 2))
        assert (t2 - t).abs().max().item() <= 1e-12 and (2 * (M - t2) / (K * R * R) - G_ref).abs().max().item() <= 1e-12
        assert (((M - t2) ** 2).mean(dim=(1, 2, 3)) - E_ref).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the step formula
# ---------------------------------------------------------------------------------------------------------------------------------
def _step_formula_before(x, m_c, m_u, coef, guidance, prediction_type, clip, x0_prev=None, noise=None):
    """`samplers.step_formula` as it was before it took a gradient, statement by statement."""
    m = m_c if m_u is None else m_u + guidance * (m_c - m_u)
    if prediction_type == "epsilon":
        x0, eps = (x - coef.sb * m) / coef.sa, m
    elif prediction_type == "v_prediction":
        x0, eps = coef.sa * x - coef.sb * m, coef.sa * m + coef.sb * x
    else:
        x0, eps = m, (x - coef.sa * m) / coef.sb
    if clip:
        x0 = x0.clamp(-1, 1)
    y = coef.c0 * x0 + coef.ce * eps if coef.cx is None else coef.cx * x + coef.c0 * x0 + coef.ce * eps
    if x0_prev is not None:
        y = y + coef.c1 * x0_prev
    if noise is not None:
        y = y + coef.cn * noise
    return y, x0


@pytest.mark.parametrize("kind", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_step_formula_with_a_gradient(kind, clip, guided):
    """grad=None: today's result, bit for bit (float32 and float64).  With a gradient, shifting (x0, eps) is shifting the model
    output: by s g for epsilon, s g / sa for v (m = sa eps - sb x0) and -(sb / sa) s g for sample prediction -- 1e-12 in fp64."""
    from stablekeypoints_amd.ldm.samplers import StepCoef, step_formula
    gen = torch.Generator().manual_seed(31)
    coef = StepCoef(0.83, 0.5577, 0.4, 0.7, 0.3, -0.2, 0.1)
    for dtype in (torch.float32, torch.float64):
        x, mc, mu, p, z, g = (torch.randn(3, 4, 5, 5, generator=gen, dtype=dtype) for _ in range(6))
        for c in (coef, coef._replace(cx=None)):
            args = (x, mc, mu if guided else None, c, 7.5, kind, clip, p, z)
            for got, want in zip(step_formula(*args), _step_formula_before(*args)):
                assert torch.equal(got, want)
    s = torch.tensor([0.0, 1.7, -0.4], dtype=torch.float64)
    sg = s.reshape(3, 1, 1, 1) * g
    shift = {"epsilon": sg, "v_prediction": sg / coef.sa, "sample": -(coef.sb / coef.sa) * sg}[kind]
    # guidance mixes m_u + w (m_c - m_u): shifting both predictions shifts the mix by the same amount
    y, x0 = step_formula(x, mc, mu if guided else None, coef, 7.5, kind, clip, p, z, grad=g, grad_scale=s)
    y2, x02 = step_formula(x, mc + shift, mu + shift if guided else None, coef, 7.5, kind, clip, p, z)
    assert (y - y2).abs().max().item() <= 1e-12 * max(1.0, y2.abs().max().item()) and (x0 - x02).abs().max().item() <= 1e-12 * max(1.0, x02.abs().max().item())
    plain = step_formula(x, mc, mu if guided else None, coef, 7.5, kind, clip, p, z)[0]
    assert torch.equal(y[0], plain[0]) and not torch.equal(y[1], plain[1])                  # a zero scale: that row is unguided


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. behaviour on the fixed inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_guidance_moves_the_keypoints_fp64():
    """The fp64 host loop at keypoint_scale 2 against 0, 4 steps at 128^2: every image's final energy is lower, the mean arg-max
    distance to the targets is <= 0.2 and <= half the unguided one.  (Recorded: E 0.012247 / 0.012215 against 0.013201 / 0.013421,
    distance 0.116 / 0.047 against 0.59 / 0.60.)"""
    _, runs = C.host64()
    _, trace, E, dist = runs[C.SCALE]
    _, trace0, E0, dist0 = runs[0.0]
    print("final energy guided", E.tolist(), "unguided", E0.tolist(), "distance guided", dist.tolist(), "unguided", dist0.tolist())
    assert len(trace) == len(trace0) == C.STEPS and torch.equal(trace[0], trace0[0])
    assert (E < E0).all()
    assert (dist <= 0.2).all() and (dist <= 0.5 * dist0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. call hygiene (float32 modules on the host route)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from stablekeypoints_amd.optimize_token import load_ldm
    model, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=C.R, decoder=True)
    return model, next(iter(controllers.values()))


def _call(tiny, **kw):
    from stablekeypoints_amd import ptp_utils
    model, controller = tiny
    emb, lat, _ = C.inputs()
    kw.setdefault("latent", lat[:, :, :8, :8].contiguous())
    return ptp_utils.text2image_ldm_stable(model, emb, controller, num_inference_steps=2, height=64, width=64, output_type="float", **kw)


def test_call_hygiene(tiny):
    model, controller = tiny
    kp = torch.tensor(C.TARGETS)
    ids = torch.tensor(C.TOKENS)
    for bad in (dict(keypoints=kp), dict(keypoint_indices=ids), dict(keypoints=kp[:, :2], keypoint_indices=ids),
                dict(keypoints=kp[:1].expand(3, -1, -1), keypoint_indices=ids), dict(keypoints=kp, keypoint_indices=[2, 7, 16]),
                dict(keypoints=kp, keypoint_indices=[2, 7, -1]), dict(keypoints=kp[..., :1], keypoint_indices=ids)):
        with pytest.raises(ValueError):
            _call(tiny, **bad)
    gen = torch.Generator().manual_seed(1)                      # a bad pair fails before anything is drawn from the generator
    state = gen.get_state()
    for bad in (dict(keypoints=kp[0]), dict(keypoints=kp[0], keypoint_indices=[2, 7, 7]), dict(keypoints=kp[0], keypoint_indices=[2, 7, 99])):
        with pytest.raises(ValueError):
            _call(tiny, latent=None, generator=gen, **bad)
    assert torch.equal(gen.get_state(), state)
    table = (model.scheduler.timesteps, model.scheduler.num_inference_steps)
    trace = []
    img, lat0 = _call(tiny, keypoints=kp, keypoint_indices=ids, keypoint_trace=trace)
    assert img.shape == (2, 3, 64, 64) and len(trace) == 2 and all(e.shape == (2,) for e in trace)
    assert model.scheduler.timesteps is table[0] and model.scheduler.num_inference_steps == table[1]
    assert controller.step_store["attn"] == [] and model.unet.__dict__["_skp_hook_controller"].step_store["attn"] == []
    assert not any(p.grad is not None for p in model.unet.parameters())
    # [K, 2] is [n, K, 2] with repeated rows
    a, _ = _call(tiny, keypoints=kp[0], keypoint_indices=ids)
    b, _ = _call(tiny, keypoints=kp[:1].expand(2, -1, -1), keypoint_indices=ids)
    assert torch.equal(a, b) and not torch.equal(a, img)
    # an empty window is the unguided "ddim" plan call; keypoint_scale 0 inside the window too (it only records the energy)
    trace0 = []
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    plan = SamplerPlan(model.scheduler, "ddim", 0.0)           # (`sampler="ddim"` with eta 0 is routed to the scheduler's own step)
    x = C.inputs()[1][:, :, :8, :8].contiguous()
    with torch.no_grad():
        for t, c in zip(*plan.plan(2)):
            x = ptp_utils.sampler_latent_step(model, controller, x, [None, C.inputs()[0]], t, 7.5, plan=plan, coef=c, x0_hist=None)
        plain = ptp_utils._latent2float(model.vae, x)
    assert (plain - _call(tiny, sampler="ddim")[0]).abs().max().item() <= 1e-5
    off, _ = _call(tiny, keypoints=kp, keypoint_indices=ids, keypoint_steps=(0, 0), keypoint_trace=trace0)
    assert torch.equal(off, plain) and trace0 == [] and not torch.equal(img, plain)
    half = []
    _call(tiny, keypoints=kp, keypoint_indices=ids, keypoint_steps=(0.5, 1.0), keypoint_trace=half)
    assert len(half) == 1


def test_without_keypoints_the_call_is_what_it_was(tiny):
    """A regression guard, not a test of the feature (it passes without the feature too): with `keypoints=None` the loop of the
    call as it was, written out on the scheduler's own step, gives the same bytes; also for a named sampler through the step
    formula as it was."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.samplers import SamplerPlan
    model, _ = tiny
    emb, lat, _ = C.inputs()
    lat = lat[:, :, :8, :8].contiguous()
    img, _ = _call(tiny)
    with torch.no_grad():
        kept = (model.scheduler.timesteps, model.scheduler.num_inference_steps)
        model.scheduler.set_timesteps(2)
        x = lat
        for t in model.scheduler.timesteps:
            x = model.scheduler.step(ptp_utils.diffusion_step(model, x, emb, t), t, x)["prev_sample"]
        model.scheduler.timesteps, model.scheduler.num_inference_steps = kept
        assert torch.equal(img, ptp_utils._latent2float(model.vae, x))
        plan = SamplerPlan(model.scheduler, "dpm++2m", 0.0)
        ts, coefs = plan.plan(2)
        x, hist = lat, None
        for t, c in zip(ts, coefs):
            m = ptp_utils.diffusion_step(model, x, emb, t)
            x, hist = _step_formula_before(x, m, None, c, 7.5, plan.prediction_type, plan.clip_sample, hist if c.c1 != 0 else None, None)
        assert torch.equal(_call(tiny, sampler="dpm++2m")[0], ptp_utils._latent2float(model.vae, x))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. exports
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_exported_and_typed():
    """include/skp_keypoints.h against `_native.KEYPOINT_SIGNATURES` with the comparison tests/test_host_logic.py applies to
    include/skp.h, the library exports both and refuses bad arguments before any launch, and the ABI version moved."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    spec = importlib.util.spec_from_file_location("_host_logic", os.path.join(ROOT, "tests", "test_host_logic.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    hdr = open(os.path.join(ROOT, "include", "skp_keypoints.h")).read()
    assert sorted(H._header_abi(hdr)) == sorted(N.KEYPOINT_SIGNATURES) == ["skp_point_loss_f32", "skp_sampler_step_kp_f32"]
    assert H._abi_mismatches(hdr, N.KEYPOINT_SIGNATURES) == []
    assert not set(N.KEYPOINT_SIGNATURES) & set(N.SIGNATURES)
    assert N.SIGNATURES["skp_sampler_step_f32"] == N.KEYPOINT_SIGNATURES["skp_sampler_step_kp_f32"][:19] + [N._vp]
    lib = N.lib()
    assert lib.skp_abi_version() == N.ABI_VERSION >= 45
    for name, argtypes in N.KEYPOINT_SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes and len(ops._plan(name)[1]) == len(argtypes) - 1
    one = 16                                                    # any non-null address: arguments are refused before a launch
    assert lib.skp_point_loss_f32(None, one, 1, 1, 8, 1.0, one, one, None) == -1
    assert lib.skp_point_loss_f32(one, one, 1, 0, 8, 1.0, one, one, None) == -1
    assert lib.skp_point_loss_f32(one, one, 1, 1, 0, 1.0, one, one, None) == -1
    assert lib.skp_point_loss_f32(one, one, 1, 1, 8, 0.0, one, one, None) == -1
    assert lib.skp_point_loss_f32(one, one, 1, 1, 40000, 1.0, one, one, None) == -2
    step = (one, one, None, None, None, one, None, 12, 1, 1.0, 0, .8, .6, 0., 1., 0., 0., 0., 0)
    assert lib.skp_sampler_step_kp_f32(*step, None, one, 3, None) == -1
    assert lib.skp_sampler_step_kp_f32(*step, one, None, 3, None) == -1
    assert lib.skp_sampler_step_kp_f32(*step, one, one, 0, None) == -1
    assert lib.skp_sampler_step_kp_f32(*step, one, one, 5, None) == -1          # 12 elements are no 5 rows
    assert "skp_point_loss.hip" in open(os.path.join(ROOT, "stablekeypoints_amd", "csrc", "Makefile")).read()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.point_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 2), 1.0)


def test_routes_are_registered():
    from stablekeypoints_amd import routes
    assert routes.ROUTES["sample.keypoints"] == {"map_point_loss": "hip", "host": "host"}
    assert set(routes.ROUTES["sample.step"]) == {"sampler_step", "host"}
    assert routes.kind("conv_in.bwd_data", "small_out") == "hip"
