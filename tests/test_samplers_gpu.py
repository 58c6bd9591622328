"""The samplers of ldm/samplers.py on the MI355X: the step kernel (csrc/skp_sampler_step.hip) against the fp64 formula with a derived
per-element bound, its aliasing / alignment / bad-argument rules, and `ptp_utils.text2image_ldm_stable(..., sampler=, eta=)` against
the same loop on an fp64 host copy of the modules.

Module tolerances follow tests/test_generate_guided_gpu.py: the error of the EAGER fp32 modules' own loop on the GPU against fp64,
times 4.  The measured figures are recorded in profiles/generate_samplers.md."""
import copy
import itertools

import pytest
import torch

import _sampler_cases as C
from _sampler_cases import SAMPLERS, STEPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the step kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _step_rows():
    """[(label, (sa, sb, cx, c0, ce, c1, cn))] in fp64: every sampler's row at the first, a middle and the last step of the 4- and the
    20-step tables (final_alpha_cumprod = alphas_cumprod[0], as the loaded models have it), and the last row into
    final_alpha_cumprod == 1 of the two solvers, where cx = 0.  Restated from the definitions (tests/_sampler_cases.py)."""
    out = []
    _, acp, final = C.schedule(False)
    for (kind, eta), n in itertools.product(SAMPLERS, (4, 20)):
        rows = C.restated_rows(kind, eta, acp, final, n)
        out += [(f"{kind} eta={eta} {n} steps step {i}", rows[i]) for i in (0, n // 2, n - 1)]
    _, acp1, final1 = C.schedule(True)
    out += [(f"{kind} 4 steps last step into a' = 1", C.restated_rows(kind, 0.0, acp1, final1, 4)[-1]) for kind in ("dpm++2m", "dpm++2m-sde")]
    assert any(r[5] != 0 and r[6] != 0 for _, r in out) and any(r[2] == 0 and r[3] == 1.0 for _, r in out)
    return out


def _ref64(x, mc, mu, g, kind, clip, row, p, z):
    """-> (y, S, x0, X0) in fp64: the formula of include/skp.h, skp_sampler_step_f32, and the magnitude sums its roundings are
    relative to, built as tests/test_generate_guided_gpu.py builds them.  `p` / `z` None: the term is absent."""
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
    if clip:
        x0 = x0.clamp(-1, 1)
    y, S = cx * x + c0 * x0 + ce * eps, abs(cx) * ax + abs(c0) * X0 + abs(ce) * E
    if p is not None:
        y, S = y + c1 * p.double(), S + abs(c1) * p.double().abs()
    if z is not None:
        y, S = y + cn * z.double(), S + abs(cn) * z.double().abs()
    return y, S, x0, X0


# Roundings on the longest chain into y, each at most 2^-24 of a magnitude that S contains: 3 for the guidance mix (difference,
# product, sum) + 3 coefficients rounded to fp32 (sa, sb and the term's own c) + 3 operations for x0 or eps (epsilon: product,
# difference, quotient; v: two products and a sum) + 1 product with c + 4 sums of the five terms = 14; the clamp rounds nothing and
# moves x0 no further than its error.  Fused multiply-adds only remove roundings.  Rounded up to the 16 of the sibling kernel's test
# (its 14 are counted the same way); x0_out has 8 of them, relative to X0.
UNITS = 16.0


@pytest.mark.parametrize("n", [1, 5, 768, 1023, 16387])
def test_sampler_step_vs_fp64(ops, n):
    """Every row x prediction type x clip x guidance x {x0_prev, noise} present or absent, on inputs of mixed scale; per element
    |y - y64| <= 16 * 2^-24 * S and |x0_out - x0_64| <= 16 * 2^-24 * X0; copies = 2 gives the copies = 1 bits twice.  Worst case
    measured on the MI355X: profiles/generate_samplers.md."""
    gen = torch.Generator().manual_seed(200 + n)
    scale = torch.tensor([0.1, 1.0, 4.0])[torch.arange(n) % 3]
    data = []
    for noise in (0.01, 1.0):
        x = torch.randn(n, generator=gen) * scale
        mc = torch.randn(n, generator=gen)
        mu = mc + noise * torch.randn(n, generator=gen)
        p = torch.randn(n, generator=gen) * scale.flip(0)
        z = torch.randn(n, generator=gen)
        data.append((noise, (x, mc, mu, p, z), tuple(t.cuda() for t in (x, mc, mu, p, z))))
    worst, worst0, count = (0.0, None), (0.0, None), 0
    for (label, row), kind, clip, g, (has_p, has_z) in itertools.product(_step_rows(), (0, 1, 2), (False, True), (None, 7.5, 0.0, -2.0),
                                                                         ((True, True), (False, False), (True, False), (False, True))):
        noise, (x, mc, mu, p, z), (xg, mcg, mug, pg, zg) = data[count % 2]                  # the two scales of m_c - m_u in turn
        count += 1
        row = tuple(row[:5]) + (row[5] if has_p else 0.0, row[6] if has_z else 0.0)         # an absent term has a zero coefficient
        kw = dict(x0_prev=pg if has_p else None, noise=zg if has_z else None, coef=row, guidance=1.0 if g is None else g,
                  prediction=kind, clip=clip)
        x0g = torch.empty(n, device="cuda")
        y = ops.sampler_step(xg, mcg, None if g is None else mug, x0_out=x0g, **kw)
        y2 = ops.sampler_step(xg, mcg, None if g is None else mug, copies=2, **kw)
        assert y.shape == (n,) and y2.shape == (2 * n,)
        assert torch.equal(y2[:n], y) and torch.equal(y2[n:], y)
        ref, S, x0, X0 = _ref64(x, mc, None if g is None else mu, g, kind, clip, row, p if has_p else None, z if has_z else None)
        where = (label, kind, clip, g, has_p, has_z, noise)
        units = ((y.cpu().double() - ref).abs() / (2.0 ** -24 * S)).max().item()
        units0 = ((x0g.cpu().double() - x0).abs() / (2.0 ** -24 * X0)).max().item()
        worst, worst0 = max(worst, (units, where)), max(worst0, (units0, where))
        assert units <= UNITS and units0 <= UNITS, (units, units0, where)
    print(f"sampler_step n={n}: worst y error {worst[0]:.2f} units of 2^-24 S at {worst[1]}; worst x0_out error {worst0[0]:.2f} "
          f"units of 2^-24 X0 at {worst0[1]} (bound {UNITS:.0f}; {count} cases)")


def test_sampler_step_aliasing_unaligned_and_determinism(ops):
    n = 1023
    gen = torch.Generator().manual_seed(19)
    x, mc, mu, p, z = (torch.randn(n, generator=gen).cuda() for _ in range(5))
    label, row = next((l, r) for l, r in _step_rows() if r[5] != 0 and r[6] != 0)           # a second-order step of the SDE solver
    for kind, clip in itertools.product((0, 1, 2), (False, True)):
        kw = dict(coef=row, guidance=7.5, prediction=kind, clip=clip)
        x0 = torch.empty(n, device="cuda")
        y = ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, x0_out=x0, **kw)
        x0b = torch.empty(n, device="cuda")
        assert torch.equal(y, ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, x0_out=x0b, **kw)) and torch.equal(x0, x0b)   # the same bits
        xa, pa = x.clone(), p.clone()
        assert ops.sampler_step(xa, mc, mu, x0_prev=pa, noise=z, out=xa, x0_out=pa, **kw) is xa               # y is x, x0_out is x0_prev
        assert torch.equal(xa, y) and torch.equal(pa, x0)
        buf, pa = torch.empty(2 * n, device="cuda"), p.clone()
        buf[:n] = x
        ops.sampler_step(buf[:n], mc, mu, x0_prev=pa, noise=z, copies=2, out=buf, x0_out=pa, **kw)            # x is the first copy
        assert torch.equal(buf[:n], y) and torch.equal(buf[n:], y) and torch.equal(pa, x0)
        # views one float past a 16-byte boundary, each pointer in turn: the scalar form, held to the same bound
        ref, S, r0, X0 = _ref64(x.cpu(), mc.cpu(), mu.cpu(), 7.5, kind, clip, row, p.cpu(), z.cpu())
        for which in range(7):
            t = [x, mc, mu, p, z]
            x0o = torch.empty(n, device="cuda")
            if which < 5:
                base = torch.empty(n + 1, device="cuda")
                base[1:] = t[which]
                t[which] = base[1:]
                assert t[which].data_ptr() % 16 == 4
                yo = ops.sampler_step(t[0], t[1], t[2], x0_prev=t[3], noise=t[4], x0_out=x0o, **kw)
            elif which == 5:
                base = torch.full((2 * n + 1,), float("nan"), device="cuda")
                yo = ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, copies=2, out=base[1:], x0_out=x0o, **kw)
                assert torch.equal(yo[:n], yo[n:]) and bool(torch.isnan(base[0]))             # the guard element is untouched
                yo = yo[:n]
            else:
                base = torch.full((n + 1,), float("nan"), device="cuda")
                x0o = base[1:]
                yo = ops.sampler_step(x, mc, mu, x0_prev=p, noise=z, x0_out=x0o, **kw)
                assert bool(torch.isnan(base[0]))
            assert ((yo.cpu().double() - ref).abs() / (2.0 ** -24 * S)).max().item() <= UNITS, (which, kind, clip)
            assert ((x0o.cpu().double() - r0).abs() / (2.0 ** -24 * X0)).max().item() <= UNITS, (which, kind, clip)
    # a buffer with a zero coefficient is not read: the history of the first step may hold anything
    nan = torch.full((n,), float("nan"), device="cuda")
    first = tuple(row[:5]) + (0.0, 0.0)
    y = ops.sampler_step(x, mc, mu, x0_prev=nan, noise=nan.clone(), coef=first, guidance=7.5, x0_out=nan)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(nan).all())
    with pytest.raises(RuntimeError):
        ops.sampler_step(x, mc[:-1], mu, coef=first)
    with pytest.raises(RuntimeError):
        ops.sampler_step(x, mc, mu, coef=first, x0_out=torch.empty(n - 1, device="cuda"))
    with pytest.raises(ValueError):
        ops.sampler_step(x, mc, mu, coef=first, prediction="velocity")
    with pytest.raises(ValueError):
        ops.sampler_step(x, mc, mu, coef=row, noise=z)              # c1 != 0 and no x0_prev
    with pytest.raises(ValueError):
        ops.sampler_step(x, mc, mu, coef=row, x0_prev=p)            # cn != 0 and no noise


def test_sampler_step_c_abi(ops):
    lib = ops.N.lib()
    buf = torch.zeros(64, device="cuda")
    p, BAD = buf.data_ptr(), -1
    co = (1.0, 0, 0.9, 0.4, 0.5, 0.6, 0.2, 0.0, 0.0, 0)        # guidance, prediction, sa, sb, cx, c0, ce, c1, cn, clip
    f = lib.skp_sampler_step_f32
    assert f(None, p, None, None, None, p, None, 4, 1, *co, None) == BAD
    assert f(p, None, None, None, None, p, None, 4, 1, *co, None) == BAD
    assert f(p, p, None, None, None, None, None, 4, 1, *co, None) == BAD
    assert f(p, p, p, p, p, p, p, 0, 1, *co, None) == BAD
    assert f(p, p, p, p, p, p, p, -4, 1, *co, None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 0, *co, None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 3, *co, None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 1, 1.0, 3, *co[2:], None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 1, 1.0, -1, *co[2:], None) == BAD
    assert f(p, p, p, None, p, p, p, 4, 1, 1.0, 0, 0.9, 0.4, 0.5, 0.6, 0.2, 0.3, 0.0, 0, None) == BAD      # c1 != 0, no x0_prev
    assert f(p, p, p, p, None, p, p, 4, 1, 1.0, 0, 0.9, 0.4, 0.5, 0.6, 0.2, 0.0, 0.3, 0, None) == BAD      # cn != 0, no noise
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(64))              # nothing was launched
    out = torch.zeros(8, device="cuda")
    assert f(p, p, None, None, None, out.data_ptr(), None, 4, 2, *co, None) == 0       # the optional pointers may all be null
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.zeros(8))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the loop: the reduced-width tree, 64^2 images (8^2 latents), 4 steps
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (unconditional embedding: None / "u16" (equal length: the doubled route) / "u24" (two forwards), samplers)
LOOP_CASES = {"plain": (None, SAMPLERS), "guided": ("u16", SAMPLERS), "guided_t24": ("u24", C.T24_SAMPLERS)}
# the batch: every sampler, unguided and guided (seeds C.BATCH_SEEDS)
BATCH_CASES = {"plain": SAMPLERS, "guided": SAMPLERS}


@pytest.fixture(scope="module")
def trees():
    """The fused pipeline on the GPU, the same modules eager on the GPU and in fp64 on the host, and for every case the single-image
    reference loops (fp64, and eager fp32 for the yardstick), computed once and only read by the tests.  The eager loops run under
    the library's fixed-summation-order convolution solvers, as the sampling call itself does."""
    from stablekeypoints_amd import ptp_utils
    from stablekeypoints_amd.ldm.pipeline import StableDiffusionPipeline
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True)
    sched, acp, final = C.schedule(False)
    assert (ldm.scheduler.clip_sample, ldm.scheduler.final_alpha_cumprod, ldm.scheduler.prediction_type) == (False, final, "epsilon")
    plain = StableDiffusionPipeline.from_pretrained("tiny", scheduler=sched, with_decoder=True)
    for k, v in ldm.unet.state_dict().items():
        assert torch.equal(v.cpu(), plain.unet.state_dict()[k]), k
    cpu64 = copy.deepcopy(plain)
    cpu64.unet.double(); cpu64.vae.double()
    eager = plain.to("cuda")
    emb = C.embeddings()
    todo = {(name, s, e, C.SINGLE_SEED) for name, (_, ss) in LOOP_CASES.items() for s, e in ss}
    todo |= {(name, s, e, seed) for name, ss in BATCH_CASES.items() for s, e in ss for seed in C.BATCH_SEEDS}
    ref = {}
    with torch.no_grad(), ptp_utils._reproducible_library_convolutions():
        for name, s, e, seed in sorted(todo):
            u = None if LOOP_CASES[name][0] is None else emb[LOOP_CASES[name][0]]
            lat, noise = C.draw(seed, C.stochastic(s, e))
            args = (acp, final, "epsilon", False, s, e, lat, emb["cond"], u, noise, C.GUIDANCE)
            r64 = C.loop(cpu64, torch.float64, "cpu", *args)
            ref[(name, s, e, seed)] = (r64, C.rel(C.loop(eager, torch.float32, "cuda", *args).cpu().double(), r64))
    return dict(ldm=ldm, ctrl=next(iter(controllers.values())), emb=emb, ref=ref, ptp=ptp_utils)


def _sample(trees, name, sampler, eta, **kw):
    from stablekeypoints_amd import routes
    unc = LOOP_CASES[name][0]
    extra = {} if unc is None else dict(uncond_embedding=trees["emb"][unc], guidance_scale=C.GUIDANCE)
    ldm, ctrl = trees["ldm"], trees["ctrl"]
    before = routes.snapshot()
    out = trees["ptp"].text2image_ldm_stable(ldm, trees["emb"]["cond"], ctrl, num_inference_steps=STEPS, height=64, width=64,
                                             output_type="float", sampler=sampler, eta=eta, **extra, **kw)
    d = routes.delta(before)
    assert d.get(("sample.step", "sampler_step"), 0) == STEPS and ("sample.step", "host") not in d, d      # once per step
    assert not ctrl.step_store["attn"]                          # the hooked store is left empty
    assert int(ldm.scheduler.timesteps[0]) == 980 and ldm.scheduler.num_inference_steps == 50             # the scheduler is untouched
    return out


@pytest.mark.parametrize("name,sampler,eta", [(name, s, e) for name, (_, ss) in LOOP_CASES.items() for s, e in ss])
def test_sampler_loop_vs_fp64_loop(trees, tune, name, sampler, eta):
    """One image, 4 steps at 64^2, latent and noise drawn from the generator: each sampler unguided, guided with contexts of equal
    length (the doubled route: one 2-row forward, the step writes both copies) and of different length (two forwards), against the
    same loop on the fp64 host copy; tolerance 4x the eager fp32 loop's own error.  Figures: profiles/generate_samplers.md."""
    tune("conv_up2", 1)                                         # as tests/test_generate_gpu.py: the 32-channel up-samplers on the own kernel
    lat, _ = C.draw(C.SINGLE_SEED, False)
    img, lat0 = _sample(trees, name, sampler, eta, generator=torch.Generator().manual_seed(C.SINGLE_SEED))
    r64, e_eager = trees["ref"][(name, sampler, eta, C.SINGLE_SEED)]
    assert img.shape == (1, 3, 64, 64) and img.is_cuda and torch.equal(lat0, lat)
    e_fused = C.rel(img.cpu().double(), r64)
    print(f"sampling tiny 4 steps 64^2 [{name}, {sampler} eta={eta}]: eager fp32 loop vs fp64 {e_eager:.3e}, fused vs fp64 "
          f"{e_fused:.3e} (bound {4 * e_eager:.3e})")
    assert e_fused <= 4 * e_eager
    again, _ = _sample(trees, name, sampler, eta, generator=torch.Generator().manual_seed(C.SINGLE_SEED))
    assert torch.equal(again, img)                              # equal seeds, equal bits


@pytest.mark.parametrize("name,sampler,eta", [(name, s, e) for name, ss in BATCH_CASES.items() for s, e in ss])
def test_sampler_batch_rows_vs_their_own_fp64_loops(trees, tune, name, sampler, eta):
    """Two images in one call: row i against its own fp64 single-image loop, bound 4x the error of the eager fp32 single-image loop
    with that generator; the single-image call with generator[i] is held to the same bound, and the two agree within the sum of
    their bounds (the rule of tests/test_generate_guided_gpu.py)."""
    tune("conv_up2", 1)
    img, lat = _sample(trees, name, sampler, eta, generator=[torch.Generator().manual_seed(s) for s in C.BATCH_SEEDS])
    assert img.shape == (2, 3, 64, 64) and lat.shape == (2, 4, 8, 8)
    for i, seed in enumerate(C.BATCH_SEEDS):
        r64, e_eager = trees["ref"][(name, sampler, eta, seed)]
        assert torch.equal(lat[i:i + 1], C.draw(seed, False)[0])
        e_row = C.rel(img[i:i + 1].cpu().double(), r64)
        one, _ = _sample(trees, name, sampler, eta, generator=torch.Generator().manual_seed(seed))
        e_one = C.rel(one.cpu().double(), r64)
        print(f"batch of 2 [{name}, {sampler} eta={eta}] row {i} (seed {seed}): eager single-image loop vs fp64 {e_eager:.3e}, fused "
              f"batched row vs fp64 {e_row:.3e}, fused single call vs fp64 {e_one:.3e} (bound {4 * e_eager:.3e})")
        assert e_row <= 4 * e_eager and e_one <= 4 * e_eager
        assert (img[i:i + 1] - one).abs().max().item() <= 8 * e_eager * r64.abs().max().item()


def test_default_call_keeps_its_route_and_bits(trees):
    """`sampler=None` and `sampler="ddim", eta=0` are the loop of `latent_step` / `guided_latent_step` on `model.scheduler.step`,
    bit for bit, and note nothing at `sample.step`."""
    from stablekeypoints_amd import ops, routes
    ldm, ctrl, emb, ptp = trees["ldm"], trees["ctrl"], trees["emb"], trees["ptp"]
    lat = torch.cat([C.draw(s, False)[0] for s in C.BATCH_SEEDS])
    kw = dict(num_inference_steps=STEPS, height=64, width=64, latent=lat, output_type="float")
    for unc in (None, "u16", "u24"):
        extra = {} if unc is None else dict(uncond_embedding=emb[unc], guidance_scale=C.GUIDANCE)
        before = routes.snapshot()
        a, _ = ptp.text2image_ldm_stable(ldm, emb["cond"], ctrl, **kw, **extra)
        b, _ = ptp.text2image_ldm_stable(ldm, emb["cond"], ctrl, sampler=None, **kw, **extra)
        c, _ = ptp.text2image_ldm_stable(ldm, emb["cond"], ctrl, sampler="ddim", eta=0.0, **kw, **extra)
        assert not [k for k in routes.delta(before) if k[0] == "sample.step"]
        sched = ldm.scheduler
        kept = (sched.timesteps, sched.num_inference_steps)
        try:
            with torch.no_grad(), ptp._reproducible_library_convolutions(), ops.up2_in_unet(True):
                sched.set_timesteps(STEPS)
                x = lat.cuda()
                context = [None if unc is None else emb[unc].cuda(), emb["cond"].cuda()]
                for t in sched.timesteps:
                    x = (ptp.latent_step(ldm, ctrl, x, context, t, C.GUIDANCE) if unc is None else
                         ptp.guided_latent_step(ldm, ctrl, x, context, t, C.GUIDANCE))
                    ctrl.reset()
                want = ptp._latent2float(ldm.vae, x)
        finally:
            sched.timesteps, sched.num_inference_steps = kept
        # (with "u16" the call keeps the 2n-row input between steps and the step kernel writes both copies: the same values)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, want), unc
