"""CPU tests of the captured sampling loop (include/skp_sampler_graph.h, `text2image_ldm_stable(capture=True)`): the header against its
table, refusals before any launch, the packed coefficient table, the graph key, and the host route of the keyword."""
import importlib.util
import os
import warnings

import numpy as np
import pytest
import torch

import _graph_cases as G
import _sampler_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["skp_axpby_dev_f32", "skp_ddim_step_dev_f32", "skp_sampler_step_dev_f32", "skp_sampler_step_kp_dev_f32", "skp_step_advance"]


def _host_logic():
    spec = importlib.util.spec_from_file_location("_host_logic", os.path.join(ROOT, "tests", "test_host_logic.py"))
    H = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(H)
    return H


def test_graph_header_agrees_with_its_table():
    """include/skp_sampler_graph.h against `_native.SAMPLER_GRAPH_SIGNATURES` with the comparison tests/test_host_logic.py applies to
    skp.h; the library exports the entries, the table is disjoint from the other four, every entry ends in the stream, the row
    width is the header's, and each device-row entry is its by-value sibling with (table, step, steps) in place of the scalars."""
    from stablekeypoints_amd import _native as N
    from stablekeypoints_amd import ops
    from stablekeypoints_amd.ldm import samplers
    H = _host_logic()
    hdr = open(os.path.join(ROOT, "include", "skp_sampler_graph.h")).read()
    abi = H._header_abi(hdr)
    assert sorted(abi) == sorted(N.SAMPLER_GRAPH_SIGNATURES) == ENTRIES
    assert H._abi_mismatches(hdr, N.SAMPLER_GRAPH_SIGNATURES) == []
    others = set(N.SIGNATURES) | set(N.KEYPOINT_SIGNATURES) | set(N.OVERLAY_SIGNATURES) | set(N.LOCATE_SIGNATURES)
    assert not set(N.SAMPLER_GRAPH_SIGNATURES) & others
    assert all(kinds[-1] == "dev:void" for _, kinds in abi.values())
    assert f"#define SKP_STEP_ROW {G.ROW}" in hdr and ops.STEP_ROW == samplers.STEP_ROW == G.ROW
    lib = N.lib()
    assert lib.skp_abi_version() == N.ABI_VERSION >= 48
    for name, argtypes in N.SAMPLER_GRAPH_SIGNATURES.items():
        assert getattr(lib, name).argtypes == argtypes and N.signature(name) is argtypes
    mk = open(os.path.join(ROOT, "stablekeypoints_amd", "csrc", "Makefile")).read()
    assert "skp_sampler_graph.h" in mk
    row = [N._pf, N._pi, N._i]                                   # const float* table, const int32_t* step, int steps

    def without_scalars(sig):
        return [t for t in sig if t is not N._f]
    assert N.SAMPLER_GRAPH_SIGNATURES["skp_axpby_dev_f32"][3:] == [N._i64] + row + [N._vp]
    assert N.SAMPLER_GRAPH_SIGNATURES["skp_ddim_step_dev_f32"] == without_scalars(N.SIGNATURES["skp_ddim_step_f32"])[:-1] + row + [N._vp]
    assert (N.SAMPLER_GRAPH_SIGNATURES["skp_sampler_step_dev_f32"]
            == without_scalars(N.SIGNATURES["skp_sampler_step_f32"])[:-1] + row + [N._vp])
    kp = without_scalars(N.KEYPOINT_SIGNATURES["skp_sampler_step_kp_f32"])
    assert N.SAMPLER_GRAPH_SIGNATURES["skp_sampler_step_kp_dev_f32"] == kp[:-4] + row + kp[-4:]


def _args(name, **over):
    """A legal argument list of a device-row entry (any non-null address: arguments are refused before a launch), edited by name."""
    one = 16
    a = {"skp_axpby_dev_f32": dict(x=one, z=one, y=one, n=4, table=one, step=one, steps=3),
         "skp_ddim_step_dev_f32": dict(x=one, m_c=one, m_u=one, y=one, n=4, copies=1, prediction=0, clip=0, table=one, step=one, steps=3),
         "skp_sampler_step_dev_f32": dict(x=one, m_c=one, m_u=one, x0_prev=one, noise=one, y=one, x0_out=one, n=4, copies=1,
                                          prediction=0, clip=0, table=one, step=one, steps=3),
         "skp_sampler_step_kp_dev_f32": dict(x=one, m_c=one, m_u=one, x0_prev=one, noise=one, y=one, x0_out=one, n=4, copies=1,
                                             prediction=0, clip=0, table=one, step=one, steps=3, g=one, gs=one, rows=2)}[name]
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values()) + [None]


def test_entries_refuse_bad_arguments_before_launching():
    """NULL `table` / `step` and a row count that is not positive are SKP_E_BADARG, and so is everything the by-value sibling
    refuses that does not depend on the coefficients."""
    from stablekeypoints_amd import _native as N
    lib = N.lib()
    BAD = -1
    assert lib.skp_step_advance(None, None) == BAD
    for name in ENTRIES[:-1]:
        f = getattr(lib, name)
        for what in (dict(table=None), dict(step=None), dict(steps=0), dict(steps=-1), dict(x=None), dict(y=None), dict(n=0), dict(n=-4)):
            assert f(*_args(name, **what)) == BAD, (name, what)
    assert lib.skp_axpby_dev_f32(*_args("skp_axpby_dev_f32", z=None)) == BAD
    assert lib.skp_axpby_dev_f32(*_args("skp_axpby_dev_f32", n=(2 ** 31 - 1) * 256 + 1)) == -2
    for name in ENTRIES[1:-1]:
        f = getattr(lib, name)
        for what in (dict(m_c=None), dict(copies=0), dict(copies=3), dict(prediction=-1), dict(prediction=3)):
            assert f(*_args(name, **what)) == BAD, (name, what)
    f = lib.skp_sampler_step_kp_dev_f32
    for what in (dict(g=None), dict(gs=None), dict(rows=0), dict(rows=3)):                   # n % rows != 0
        assert f(*_args("skp_sampler_step_kp_dev_f32", **what)) == BAD, what


def test_wrappers_refuse_host_tensors_and_wrong_rows():
    from stablekeypoints_amd import ops
    x = torch.zeros(8)
    table, step = torch.zeros(3, G.ROW), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sampler_step_dev(x, x, table=table, step=step, steps=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ddim_step_dev(x, x, table=table, step=step, steps=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.axpby_dev(x, x, table=table, step=step, steps=3)
    with pytest.raises(RuntimeError, match="one int32 on the device"):
        ops.step_advance(step)
    for bad in (dict(table=table), dict(table=None), dict(step=step)):
        with pytest.raises(RuntimeError):
            ops._step_row("t", **{**dict(table=table, step=step, steps=3), **bad})


def test_packed_table_is_the_rows_rounded_once():
    """`pack_step_table` of a plan's `StepCoef` rows against the rows restated in tests/_sampler_cases.py, each number rounded to
    float32 once by the C conversion; column 7 is the guidance scale; a None `cx` is stored as 0."""
    from stablekeypoints_amd.ldm.samplers import SamplerPlan, StepCoef, pack_step_table
    sched, acp, final = S.schedule(False)
    for (kind, eta), n in ((k, n) for k in S.SAMPLERS for n in (4, 6, 20)):
        coefs = SamplerPlan(sched, kind, eta).plan(n)[1]
        t = pack_step_table(coefs, 7.3)
        assert t.dtype == torch.float32 and tuple(t.shape) == (n, G.ROW) and not t.is_cuda
        want = np.array([[G.f32(v) for v in row] + [G.f32(7.3)] for row in S.restated_rows(kind, eta, acp, final, n)], dtype=np.float32)
        restated64 = np.array([list(row) for row in S.restated_rows(kind, eta, acp, final, n)])
        assert np.allclose(np.array([list(c) for c in coefs]), restated64, rtol=1e-12, atol=1e-15)
        assert np.array_equal(t.numpy(), np.array([[G.f32(v) for v in c] + [G.f32(7.3)] for c in coefs], dtype=np.float32))
        assert np.allclose(t.numpy(), want, rtol=2.0 ** -23, atol=1e-30)
    t = pack_step_table([StepCoef(0.9, 0.4, None, 0.8, 0.6, 0, 0)])
    assert t.tolist() == [[G.f32(0.9), G.f32(0.4), 0.0, G.f32(0.8), G.f32(0.6), 0.0, 0.0, 1.0]]


def test_default_rows_are_the_schedulers_numbers():
    """The rows of the call without a sampler: what `DDIMScheduler.step` hands `ops.axpby` (c1 = pa / sa, c2 = pb - pa sb / sa) in
    columns cx / ce, or (pa, pb) in columns c0 / ce for the DDIM step kernel."""
    from stablekeypoints_amd import ptp_utils
    sched, _, _ = S.schedule(False)
    sched.set_timesteps(5)
    for kind in ("axpby", "ddim_step"):
        rows = ptp_utils._default_rows(sched, sched.timesteps, kind)
        assert len(rows) == 5
        for t, r in zip(sched.timesteps, rows):
            sa, sb, pa, pb = sched._coefficients(t)
            assert (r.sa, r.sb, r.c1, r.cn) == (sa, sb, 0.0, 0.0)
            assert (r.cx, r.ce) == (pa / sa, pb - pa * sb / sa) if kind == "axpby" else (r.c0, r.ce) == (pa, pb)


def test_key_separates_every_configuration():
    from stablekeypoints_amd import ptp_utils
    base, others = G.key_configurations()
    keys = [ptp_utils.sample_graph_key(**c) for c in [base] + others]
    assert len(set(keys)) == len(keys) and all(hash(k) is not None for k in keys)
    assert ptp_utils.sample_graph_key(**base) == keys[0]
    assert keys[0][:-1] == ptp_utils.sample_graph_key(**dict(base, tag=(("w", 9),)))[:-1]     # the tag is the last field
    cache = ptp_utils.SampleGraphs()
    cache.entries[keys[0]] = "eager"
    cache.last = "eager"
    cache.clear()
    assert cache.keys() == [] and cache.last is None


class _OwnCallback:
    def step_callback(self, x):
        return x

    def reset(self):
        pass


def test_step_callback_override_is_detected():
    from stablekeypoints_amd import ptp_utils
    assert not ptp_utils._overrides_step_callback(None)
    assert not ptp_utils._overrides_step_callback(ptp_utils.AttentionStore())
    assert ptp_utils._overrides_step_callback(_OwnCallback())

    class Sub(ptp_utils.AttentionStore):
        def step_callback(self, x_t):
            return x_t
    assert ptp_utils._overrides_step_callback(Sub())


@pytest.fixture(scope="module")
def host_model():
    from stablekeypoints_amd.optimize_token import load_ldm
    ldm, controllers, _ = load_ldm("cpu", "tiny", feature_upsample_res=32, decoder=True)
    return ldm, next(iter(controllers.values()))


@pytest.mark.parametrize("sampler,unc", [(None, None), ("dpm++2m-sde", "u16")])
def test_capture_on_host_modules_is_the_host_route(host_model, sampler, unc):
    """`capture=True` on CPU modules: the bits of `capture=False`, `sample.loop` / `host` once per step, no warning, nothing kept."""
    from stablekeypoints_amd import ptp_utils, routes
    ldm, ctrl = host_model
    emb = S.embeddings()
    kw = dict(num_inference_steps=3, height=64, width=64, output_type="float", sampler=sampler)
    if unc is not None:
        kw.update(uncond_embedding=emb[unc], guidance_scale=G.GUIDANCE)
    before = routes.snapshot()
    a, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, generator=torch.Generator().manual_seed(50), **kw)
    assert not [k for k in routes.delta(before) if k[0] == "sample.loop"]                    # the call as it always was notes nothing
    before = routes.snapshot()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b, _ = ptp_utils.text2image_ldm_stable(ldm, emb["cond"], ctrl, generator=torch.Generator().manual_seed(50), capture=True, **kw)
    d = routes.delta(before)
    assert torch.equal(a, b)
    assert {k: v for k, v in d.items() if k[0] == "sample.loop"} == {("sample.loop", "host"): 3}
    assert ptp_utils.sample_graphs(ldm).keys() == []
    assert int(ldm.scheduler.timesteps[0]) == 980 and ldm.scheduler.num_inference_steps == 50
