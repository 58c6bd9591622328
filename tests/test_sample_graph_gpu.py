"""The captured sampling loop on the MI355X: the device-row step kernels (include/skp_sampler_graph.h) against their by-value
siblings bit for bit, and `text2image_ldm_stable(capture=True)` against `capture=False` on the same model, seeds and arguments.

Expectation of the loop tests: equal bits.  Two identical eager calls give equal bits on this tree, a replay launches
the kernels of the eager step on the same values, and every per-step number the kernels read from device tables is the float the
eager launch receives in its argument list."""
import itertools
import warnings

import pytest
import torch

import _graph_cases as G
import _keypoint_cases as K
import _sampler_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from stablekeypoints_amd import ops as o
    o.N.lib()
    return o


def _counter(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_of(n):
    return 3 if n % 3 == 0 else 1


def _data(n, seed):
    """n elements as [rows, n / rows] (rows = 3 where 3 divides n: a scale of the gradient term per row) -> x, m_c, m_u, x0_prev, the
    noise of EVERY step [TABLE_ROWS, rows, n / rows] (the kernel picks row *step), the gradient and its scales [rows]."""
    gen = torch.Generator().manual_seed(seed)
    rows = _rows_of(n)
    shape = (rows, n // rows)
    scale = torch.tensor([0.1, 1.0, 4.0])[torch.arange(n) % 3].reshape(shape)
    x = torch.randn(shape, generator=gen) * scale
    mc = torch.randn(shape, generator=gen)
    mu = mc + 0.5 * torch.randn(shape, generator=gen)
    p = torch.randn(shape, generator=gen) * scale.flip(1)
    z = torch.randn((G.TABLE_ROWS,) + shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    gs = torch.tensor([0.7, -1.3, 2.1][:rows])
    return tuple(t.cuda() for t in (x, mc, mu, p, z, g, gs))


@pytest.mark.parametrize("n", G.SIZES)
def test_sampler_step_dev_has_the_bits_of_sampler_step(ops, n):
    """Every sampler's row at its first, a middle and its last step, read as row *step = 0, 3, 6 of a 7-row table whose other
    rows are NaN, x prediction type x clip x guided or not x copies x with and without the gradient term: y, both copies and
    x0_out equal the by-value entry's bits.  The sibling gets the row's noise and, as its rule says, no pointer where the
    coefficient is 0; the device-row entry always gets both buffers and the whole noise."""
    x, mc, mu, p, z, g, gs = _data(n, 300 + n)
    rows = _rows_of(n)
    count = 0
    for (label, pos, row), kind, clip, guided, copies, kp in itertools.product(G.sampler_rows(), (0, 1, 2), (False, True),
                                                                               (False, True), (1, 2), (False, True)):
        at = G.AT[pos]
        table, step = G.table_with(row, at).cuda(), _counter(at)
        extra = dict(grad=g, grad_scale=gs) if kp else {}
        common = dict(prediction=kind, clip=clip, copies=copies, **extra)
        x0a, x0b = torch.empty_like(x), torch.empty_like(x)
        want = ops.sampler_step(x, mc, mu if guided else None, x0_prev=p if row[5] != 0 else None, noise=z[at] if row[6] != 0 else None,
                                coef=row, guidance=G.GUIDANCE, x0_out=x0a, **common)
        got = ops.sampler_step_dev(x, mc, mu if guided else None, x0_prev=p, noise=z, table=table, step=step, steps=G.TABLE_ROWS,
                                   x0_out=x0b, **common)
        assert got.shape == want.shape == (copies * rows, n // rows)
        assert torch.equal(got, want) and torch.equal(x0b, x0a), (label, kind, clip, guided, copies, kp)
        assert int(step.item()) == at                                   # no step kernel writes the counter
        count += 1
    assert count == len(G.sampler_rows()) * 48


@pytest.mark.parametrize("n", G.SIZES)
def test_ddim_step_dev_and_axpby_dev_have_their_siblings_bits(ops, n):
    """The DDIM step with (sa, sb, pa, pb, guidance) = columns (0, 1, 3, 4, 7) and the plain update with (a, b) = columns (2, 4) of
    row *step, at the three positions, for every prediction type, clip, guidance and copies."""
    x, mc, mu = _data(n, 400 + n)[:3]
    for (label, pos, row), kind, clip, guided, copies in itertools.product(G.sampler_rows(), (0, 1, 2), (False, True), (False, True),
                                                                           (1, 2)):
        at = G.AT[pos]
        table, step = G.table_with(row, at).cuda(), _counter(at)
        want = ops.ddim_step(x, mc, mu if guided else None, sa=row[0], sb=row[1], pa=row[3], pb=row[4], guidance=G.GUIDANCE,
                             prediction=kind, clip=clip, copies=copies)
        got = ops.ddim_step_dev(x, mc, mu if guided else None, table=table, step=step, steps=G.TABLE_ROWS, prediction=kind, clip=clip,
                                copies=copies)
        assert got.shape == want.shape and torch.equal(got, want), (label, kind, clip, guided, copies)
    for label, pos, row in G.sampler_rows():
        at = G.AT[pos]
        table, step = G.table_with(row, at).cuda(), _counter(at)
        want = ops.axpby(x, mc, row[2], row[4])
        assert torch.equal(ops.axpby_dev(x, mc, table=table, step=step, steps=G.TABLE_ROWS), want), label
        xa = x.clone()
        assert ops.axpby_dev(xa, mc, table=table, step=step, steps=G.TABLE_ROWS, out=xa) is xa and torch.equal(xa, want)     # y is x


def test_zero_coefficients_leave_their_buffers_unread(ops):
    """A row with c1 = 0 or cn = 0 against x0_prev and noise buffers full of NaN: the result is finite and equals the sibling's
    with NULL pointers -- at every position of the counter, so the noise row that is skipped is the indexed one."""
    x, mc, mu, p, z, g, gs = _data(1023, 77)
    nan_p, nan_z = torch.full_like(p, float("nan")), torch.full_like(z, float("nan"))
    label, _, full = next(r for r in G.sampler_rows() if r[2][5] != 0 and r[2][6] != 0)        # a second-order step of the SDE solver
    for at, (zero_p, zero_z), kp in itertools.product(G.AT, ((True, True), (True, False), (False, True)), (False, True)):
        row = tuple(full[:5]) + (0.0 if zero_p else full[5], 0.0 if zero_z else full[6])
        table, step = G.table_with(row, at).cuda(), _counter(at)
        extra = dict(grad=g, grad_scale=gs) if kp else {}
        x0a, x0b = torch.empty_like(x), torch.empty_like(x)
        want = ops.sampler_step(x, mc, mu, x0_prev=None if zero_p else p, noise=None if zero_z else z[at], coef=row,
                                guidance=G.GUIDANCE, x0_out=x0a, **extra)
        got = ops.sampler_step_dev(x, mc, mu, x0_prev=nan_p if zero_p else p, noise=nan_z if zero_z else z, table=table, step=step,
                                   steps=G.TABLE_ROWS, x0_out=x0b, **extra)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want) and torch.equal(x0b, x0a), (at, zero_p, zero_z, kp)
    # the history updated in place while it is not read: x0_out is x0_prev, which holds NaN
    row = tuple(full[:5]) + (0.0, full[6])
    hist = nan_p.clone()
    ops.sampler_step_dev(x, mc, mu, x0_prev=hist, noise=z, table=G.table_with(row, 3).cuda(), step=_counter(3), steps=G.TABLE_ROWS,
                         x0_out=hist)
    assert bool(torch.isfinite(hist).all())


def test_aliasing_unaligned_pointers_and_the_counters_range(ops):
    n, rows = 1023, 3
    m = n // rows
    x, mc, mu, p, z, g, gs = _data(n, 19)
    label, _, row = next(r for r in G.sampler_rows() if r[2][5] != 0 and r[2][6] != 0)
    at = 3
    table, step = G.table_with(row, at).cuda(), _counter(at)
    row_kw = dict(table=table, step=step, steps=G.TABLE_ROWS)
    for kind, clip, kp in itertools.product((0, 1, 2), (False, True), (False, True)):
        kw = dict(prediction=kind, clip=clip, **(dict(grad=g, grad_scale=gs) if kp else {}))
        x0 = torch.empty_like(x)
        y = ops.sampler_step(x, mc, mu, x0_prev=p, noise=z[at], coef=row, guidance=G.GUIDANCE, x0_out=x0, **kw)
        xa, pa = x.clone(), p.clone()
        assert ops.sampler_step_dev(xa, mc, mu, x0_prev=pa, noise=z, out=xa, x0_out=pa, **row_kw, **kw) is xa     # y is x, x0_out is x0_prev
        assert torch.equal(xa, y) and torch.equal(pa, x0)
        buf, pa = torch.empty(2 * rows, m, device="cuda"), p.clone()
        buf[:rows] = x
        ops.sampler_step_dev(buf[:rows], mc, mu, x0_prev=pa, noise=z, copies=2, out=buf, x0_out=pa, **row_kw, **kw)   # x is the first copy
        assert torch.equal(buf[:rows], y) and torch.equal(buf[rows:], y) and torch.equal(pa, x0)
        # views one float past a 16-byte boundary, each pointer in turn (the noise: its base): the sibling's rule is the scalar
        # form, and the bits do not depend on the form
        for which in range(7):
            t = [x, mc, mu, p, z]
            x0o = torch.empty_like(x)
            if which < 5:
                base = torch.empty(t[which].numel() + 1, device="cuda")
                base[1:] = t[which].reshape(-1)
                t[which] = base[1:].reshape(t[which].shape)
                assert t[which].data_ptr() % 16 == 4 and t[which].is_contiguous()
                yo = ops.sampler_step_dev(t[0], t[1], t[2], x0_prev=t[3], noise=t[4], x0_out=x0o, **row_kw, **kw)
            elif which == 5:
                base = torch.full((2 * n + 1,), float("nan"), device="cuda")
                yo = ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z, copies=2, out=base[1:].reshape(2 * rows, m), x0_out=x0o,
                                          **row_kw, **kw)
                assert torch.equal(yo[:rows], yo[rows:]) and bool(torch.isnan(base[0]))       # the guard element is untouched
                yo = yo[:rows]
            else:
                base = torch.full((n + 1,), float("nan"), device="cuda")
                x0o = base[1:].reshape(rows, m)
                yo = ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z, x0_out=x0o, **row_kw, **kw)
                assert bool(torch.isnan(base[0]))
            assert torch.equal(yo, y) and torch.equal(x0o, x0), (which, kind, clip, kp)
    # a counter outside the table: nothing is read or written (the guard the host cannot apply at launch)
    for bad in (-1, G.TABLE_ROWS):
        out, x0o = torch.full_like(x, 3.0), torch.full_like(x, 5.0)
        ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z, out=out, x0_out=x0o, table=table, step=_counter(bad), steps=G.TABLE_ROWS)
        ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z, out=out, x0_out=x0o, table=table, step=_counter(bad), steps=G.TABLE_ROWS,
                             grad=g, grad_scale=gs)
        ops.ddim_step_dev(x, mc, mu, out=out, table=table, step=_counter(bad), steps=G.TABLE_ROWS)
        ops.axpby_dev(x, mc, out=out, table=table, step=_counter(bad), steps=G.TABLE_ROWS)
        assert bool((out == 3.0).all()) and bool((x0o == 5.0).all())
    # the wrapper holds the table to the plan: fewer rows than steps is refused on the host
    with pytest.raises(ValueError):
        ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z, table=table, step=step, steps=G.TABLE_ROWS + 1)
    with pytest.raises(ValueError):
        ops.sampler_step_dev(x, mc, mu, x0_prev=p, noise=z[:3], table=table, step=step, steps=G.TABLE_ROWS)
    with pytest.raises(ValueError):
        ops.ddim_step_dev(x, mc, mu, table=table[:2], step=step, steps=3)
    with pytest.raises(RuntimeError):
        ops.sampler_step_dev(x, mc, mu, table=table, step=step.long(), steps=G.TABLE_ROWS)
    with pytest.raises(RuntimeError):
        ops.sampler_step_dev(x, mc, mu, table=table[:, :7], step=step, steps=G.TABLE_ROWS)


def test_c_abi_refusals_and_the_counter(ops):
    lib = ops.N.lib()
    buf = torch.zeros(64, device="cuda")
    cnt = _counter(0)
    p, c, BAD = buf.data_ptr(), cnt.data_ptr(), -1
    f = lib.skp_sampler_step_dev_f32
    assert f(p, p, p, p, p, p, p, 4, 1, 0, 0, None, c, 3, None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 1, 0, 0, p, None, 3, None) == BAD
    assert f(p, p, p, p, p, p, p, 4, 1, 0, 0, p, c, 0, None) == BAD
    assert lib.skp_sampler_step_kp_dev_f32(p, p, p, p, p, p, p, 4, 1, 0, 0, None, c, 3, p, p, 1, None) == BAD
    assert lib.skp_ddim_step_dev_f32(p, p, p, p, 4, 1, 0, 0, p, None, 3, None) == BAD
    assert lib.skp_axpby_dev_f32(p, p, p, 4, None, c, 3, None) == BAD
    assert lib.skp_step_advance(None, None) == BAD
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.zeros(64)) and int(cnt.item()) == 0               # nothing was launched
    for want in (1, 2):
        assert ops.step_advance(cnt) is cnt and int(cnt.item()) == want


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------------------------------------------------------
class _Keep:
    """A controller that keeps the latents of the last step (its own `step_callback`: such a call stays on eager launches)."""
    last = None

    def step_callback(self, x):
        self.last = x
        return x

    def reset(self):
        pass


@pytest.fixture(scope="module")
def models():
    """The fused reduced-width pipeline on the GPU per prediction type, made on first use and shared."""
    from stablekeypoints_amd.optimize_token import load_ldm
    made = {}

    def get(prediction):
        if prediction not in made:
            ldm, controllers, _ = load_ldm("cuda", "tiny", feature_upsample_res=32, decoder=True, prediction_type=prediction)
            made[prediction] = (ldm, next(iter(controllers.values())))
        return made[prediction]
    return get


def _own_warnings(seen):
    return [str(w.message) for w in seen if "capture=True" in str(w.message)]


def _loop_counts(d):
    return {k[1]: v for k, v in d.items() if k[0] == "sample.loop"}


def _pair(ldm, ctrl, emb, make_kw, steps, expect_graph=True):
    """The eager call (with a controller that keeps the final latents) and the captured call with the same arguments ->
    (image, final latents) of each.  The captured call must replay exactly steps - 2 steps and run 2 on eager launches, so a
    silent fallback fails here; its final latents are the static buffer the replays wrote."""
    from stablekeypoints_amd import ptp_utils, routes
    keep = _Keep()
    img0, _ = ptp_utils.text2image_ldm_stable(ldm, emb, keep, num_inference_steps=steps, output_type="float", **make_kw())
    before = routes.snapshot()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        img1, _ = ptp_utils.text2image_ldm_stable(ldm, emb, ctrl, num_inference_steps=steps, output_type="float", capture=True,
                                                  **make_kw())
    d = routes.delta(before)
    assert not _own_warnings(seen), _own_warnings(seen)
    if expect_graph:
        assert _loop_counts(d) == {"graph": steps - 2, "eager": 2}, d
    cache = ptp_utils.sample_graphs(ldm)
    lat1 = cache.entries[cache.last_key].lat[:keep.last.shape[0]]
    assert not ctrl.step_store["attn"]                          # the hooked store is left empty
    assert int(ldm.scheduler.timesteps[0]) == 980 and ldm.scheduler.num_inference_steps == 50             # the scheduler is untouched
    return (img0, keep.last), (img1, lat1), d


@pytest.mark.parametrize("name", list(G.LOOP_CASES))
def test_captured_call_has_the_bits_of_the_eager_call(models, tune, name):
    """Every case of tests/_graph_cases.py, 6 steps at 64^2: equal bits in the final latents and in the image; the named samplers
    note their step once per step, replays included."""
    sampler, eta, unc, seeds, prediction = G.LOOP_CASES[name]
    ldm, ctrl = models(prediction)
    tune("conv_up2", 1)                                         # as tests/test_samplers_gpu.py: the 32-channel up-samplers on the own kernel
    emb = S.embeddings()

    def make_kw():
        gens = [torch.Generator().manual_seed(s) for s in seeds]
        kw = dict(height=64, width=64, sampler=sampler, eta=eta, generator=gens if len(gens) > 1 else gens[0])
        if unc is not None:
            kw.update(uncond_embedding=emb[unc], guidance_scale=S.V_GUIDED_GUIDANCE if prediction != "epsilon" else G.GUIDANCE)
        return kw
    (img0, lat0), (img1, lat1), d = _pair(ldm, ctrl, emb["cond"], make_kw, G.STEPS)
    assert img0.shape == (len(seeds), 3, 64, 64) and lat0.shape == (len(seeds), 4, 8, 8)
    assert torch.equal(lat1, lat0), f"{name}: final latents differ by {(lat1 - lat0).abs().max().item():.3e}"
    assert torch.equal(img1, img0), f"{name}: images differ by {(img1 - img0).abs().max().item():.3e}"
    named = sampler is not None and not (sampler == "ddim" and eta == 0)
    assert d.get(("sample.step", "sampler_step"), 0) == (G.STEPS if named else 0)


@pytest.mark.parametrize("unc,sampler", [(None, None), ("u16", "dpm++2m")])
def test_keypoint_guidance_runs_both_graphs_in_one_call(models, tune, unc, sampler):
    """Keypoints with keypoint_steps = (0, 0.5) over 6 steps at 128^2, two images: steps 0 and 1 on eager launches, step 2 a replay of
    the guided graph, steps 3 .. 5 replays of the unguided one -- equal bits in latents, image and the traced energies."""
    ldm, ctrl = models("epsilon")
    tune("conv_up2", 1)
    emb, lat, kp = K.inputs()
    traces = []

    def make_kw():
        traces.append([])
        kw = dict(height=128, width=128, latent=lat, keypoints=kp, keypoint_indices=torch.tensor(K.TOKENS), keypoint_scale=K.SCALE,
                  keypoint_sigma=K.SIGMA, keypoint_steps=(0.0, 0.5), keypoint_trace=traces[-1], sampler=sampler)
        if unc is not None:
            kw.update(uncond_embedding=S.embeddings()[unc], guidance_scale=2.0)
        return kw
    (img0, lat0), (img1, lat1), d = _pair(ldm, ctrl, emb, make_kw, G.STEPS)
    assert torch.equal(lat1, lat0), f"final latents differ by {(lat1 - lat0).abs().max().item():.3e}"
    assert torch.equal(img1, img0)
    assert len(traces[0]) == len(traces[1]) == 3 and all(torch.equal(a, b) for a, b in zip(*traces))
    assert d.get(("sample.keypoints", "map_point_loss")) == 3 and d.get(("sample.step", "sampler_step")) == G.STEPS
    from stablekeypoints_amd import ptp_utils
    cache = ptp_utils.sample_graphs(ldm)
    assert sorted(cache.entries[cache.last_key].graphs) == ["kp", "plain"]


def test_three_calls_on_one_key_leave_nothing_stale(models, tune):
    """Three calls in a row with another embedding, seed, guidance scale, step count (6, 4, 8) and eta: each equals its own eager
    call, and the second and third find the recorded step."""
    from stablekeypoints_amd import ptp_utils
    ldm, ctrl = models("epsilon")
    tune("conv_up2", 1)
    cache = ptp_utils.sample_graphs(ldm)
    cache.clear()
    for k, (steps, eta, seed, emb_seed, guidance) in enumerate(G.STALE_CALLS):
        g = torch.Generator().manual_seed(emb_seed)
        cond, unc = torch.randn(1, 16, 768, generator=g), torch.randn(1, 16, 768, generator=g)

        def make_kw():
            return dict(height=64, width=64, sampler="ddim", eta=eta, generator=torch.Generator().manual_seed(seed), uncond_embedding=unc,
                        guidance_scale=guidance)
        hits = cache.hits
        (img0, lat0), (img1, lat1), _ = _pair(ldm, ctrl, cond, make_kw, steps)
        assert torch.equal(lat1, lat0) and torch.equal(img1, img0), k
        assert cache.last == ("miss" if k == 0 else "hit") and cache.hits == hits + (k > 0) and len(cache.keys()) == 1, k


def test_a_changed_weight_retires_the_graph(models, tune):
    from stablekeypoints_amd import ptp_utils
    ldm, ctrl = models("epsilon")
    tune("conv_up2", 1)
    cache = ptp_utils.sample_graphs(ldm)
    emb = S.embeddings()

    def make_kw():
        return dict(height=64, width=64, sampler="dpm++2m", generator=torch.Generator().manual_seed(50))
    (img_a, _), (img_b, _), _ = _pair(ldm, ctrl, emb["cond"], make_kw, G.STEPS)
    assert torch.equal(img_a, img_b)
    old = cache.last_key
    w = ldm.unet.down_blocks[0].resnets[0].conv1.weight
    saved = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.25)
        (img0, lat0), (img1, lat1), _ = _pair(ldm, ctrl, emb["cond"], make_kw, G.STEPS)
        assert cache.last == "miss" and cache.last_key != old and cache.last_key[:-1] == old[:-1]
        assert old not in cache.entries                         # the old key is gone, with the filters its graph held
        assert torch.equal(lat1, lat0) and torch.equal(img1, img0)
        assert not torch.equal(img0, img_a)                     # (the weight mattered)
    finally:
        with torch.no_grad():
            w.copy_(saved)


def test_calls_that_stay_on_eager_launches(models, tune):
    """Two steps: eager, no warning, nothing recorded.  A controller with its own step_callback: eager, one warning."""
    from stablekeypoints_amd import ptp_utils, routes
    ldm, ctrl = models("epsilon")
    tune("conv_up2", 1)
    emb = S.embeddings()
    cache = ptp_utils.sample_graphs(ldm)
    kw = dict(height=64, width=64, sampler="dpm++2m", output_type="float")
    want, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, num_inference_steps=2, generator=torch.Generator().manual_seed(50), **kw)
    before, misses = routes.snapshot(), cache.misses
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, num_inference_steps=2, capture=True,
                                                 generator=torch.Generator().manual_seed(50), **kw)
    assert not _own_warnings(seen)
    assert torch.equal(got, want) and _loop_counts(routes.delta(before)) == {"eager": 2} and cache.misses == misses
    want, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, num_inference_steps=5, generator=torch.Generator().manual_seed(50), **kw)
    before = routes.snapshot()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], _Keep(), num_inference_steps=5, capture=True,
                                                 generator=torch.Generator().manual_seed(50), **kw)
    assert len(_own_warnings(seen)) == 1 and "step_callback" in _own_warnings(seen)[0]
    assert torch.equal(got, want) and _loop_counts(routes.delta(before)) == {"eager": 5} and cache.misses == misses
