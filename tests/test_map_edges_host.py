"""CPU half of the attention-map edge tests: the logit families of tests/_map_cases.py have their stated property at every shape
the GPU tests use, no plane of a reference is so small that the metric would leave it out, the fp32 reference is sane, the table
of variants reaches every plan value it exists for, and the restated launch plans agree with the library's host queries over a
sweep of shapes.  Nothing here touches a kernel."""
import itertools

import pytest
import torch

import _map_cases as A


@pytest.mark.parametrize("v,family", A.CASES, ids=[f"{v['name']}-{f}" for v, f in A.CASES])
def test_family_has_its_property_and_no_plane_is_left_out(v, family):
    """The family's property on the fp64 reference; every M64[b,t] plane maximum >= 1e-30 and every gradient plane maximum
    >= 1e-3 of the case's largest; the fp32 reference finite and summing to 1 over tokens within 1e-5; pad columns 0."""
    c = A.case(v, family)
    ok, what = A.check_property(family, c)
    print(f"{v['name']} {family}: {what}")
    assert ok, f"{family} on {v['name']}: {what}"
    found = A.input_conditions(c)
    print(f"{v['name']} {family}: smallest plane maximum " + ", ".join(f"{k} {x:.2e}" for k, x in found.items()),
          "| fp32 reference error " + ", ".join(f"{k} {x:.2e}" for k, x in c.err32.items()))
    # the yardstick must resolve what it measures: a reference error near 1 would let any result pass
    for name, e32 in c.err32.items():
        if name == "dS_spike":
            assert e32 <= c.spike_bound and 0 < c.spike_bound < 1e-3, (e32, c.spike_bound)
        else:
            assert e32 < 1e-3, f"the fp32 reference's own {name} error is {e32:.2e}"
    if family in ("spike_first", "spike_last") and v["kind"] == "S" and v["T"] > 1 and not v["rows"]:
        assert c.spike is not None
    for ref in (c.ref32, c.ref64):
        assert all(A._finite(x) for x in ref.values())
        assert (ref["M"].sum(1) - 1).abs().max().item() <= 1e-5
    if c.S is not None:
        assert all(S.dtype == torch.float32 and S.shape[-1] == A.nt_of(v["T"]) and not S[..., v["T"]:].any() for S in c.S)
    if c.sel is not None:
        assert all(len(set(row)) == v["K"] and 0 <= min(row) and max(row) < v["T"] for row in c.sel.tolist())


def test_seam_gradient_sits_on_the_seams_only():
    v = A.BY_NAME["sweep-s32-R128-T77-K32-3bands"]
    _, sel, G = A.make_grad(v)
    assert A.band_rows(128, 3) == [43, 86] and v["bands"] == 3
    rows = G[0, 0].abs().sum(1).nonzero().flatten().tolist()
    assert rows == [0, 42, 43, 64, 85, 86, 127]
    assert G[0, 0, 0].nonzero().flatten().tolist() == [0, 64, 127] and G[0, 0, 64].nonzero().flatten().tolist() == [0, 127]
    vals = G[G != 0]
    assert vals.unique().numel() == vals.numel() and (G[:, :, 43] != 0).all() and (G[:, :, 42] != 0).all()


@pytest.mark.parametrize("v", A.VARIANTS, ids=[v["name"] for v in A.VARIANTS])
def test_variant_shape_reaches_its_launch_plan(v, tune):
    """The table of variants against the restated plans and the library's own queries (host code of libskp_hip.so: no GPU)."""
    from stablekeypoints_amd import ops
    for key, value in v["tune"].items():
        tune(key, value)
    facts = A.assert_plan(ops, v)
    print(v["name"], {k: x for k, x in facts.items() if k in v["reach"] or k in ("fwd", "bwd", "nt")})


def test_every_listed_plan_value_is_reached():
    """Each NT, quad on and off, both tile forms with and without a ragged end, both slice widths, each register class alone and
    mixed, band counts 1 and > 1, chunks with and without a selected token: at least one variant each (a variant's own `reach` is
    proven by test_variant_shape_reaches_its_launch_plan)."""
    V = A.VARIANTS
    facts = {v["name"]: A.plan_facts(v, A.make_grad(v)[1]) for v in V}

    def has(**want):
        return any(all(f.get(k) == x for k, x in want.items()) for f in facts.values())
    narrow = [n for name, f in facts.items() if f["fwd"] != "map_wide" or f["bwd"] in ("map_dense", "map_dense_groups")
              for n in f["nt"]]
    assert set(narrow) == {16, 32, 48, 64, 80, 96, 112, 128}
    for route in ("map_fused", "map_groups", "map_wide"):
        assert has(fwd=route)
    for route in ("map_dense", "map_dense_groups", "map_col", "map_tok"):
        assert has(bwd=route)
    assert has(quad=(1,)) and has(quad=(0,)) and has(quad=(1, 0))
    assert any(f["tile"][0] == "rows" and f["tile"][2] for f in facts.values())
    assert any(f["tile"][0] == "rows" and not f["tile"][2] and f["idle_lanes"] for f in facts.values())      # 256 % R != 0
    assert has(tile=("segs", 2, True)) and has(tile=("segs", 2, False), quad=(1,))
    assert has(fwd="map_wide", sw=32) and has(fwd="map_wide", sw=64) and has(fwd="map_wide", threads=512)
    assert has(fwd="map_groups", wide_ok=False) and has(fwd="map_groups", wide_ok=True)
    for cls in (0, 1, 2):
        assert has(bwd="map_tok", cls={cls})
    assert has(bwd="map_tok", cls={0, 1, 2})
    bands = {nb for f in facts.values() if f["bwd"] == "map_tok" for nb in f["bands"].values()}
    assert {1, 2, 3, 4, 16} <= bands
    assert has(bwd="map_col", chunks=("with", "without")) and has(bwd="map_col", chunks=("with",))
    assert has(bwd="map_col", one_chunk=True) and has(bwd="map_col", last_chunk_empty=True)
    assert has(k2=(4,)) and has(k2=(2,)) and has(k2=(4, 4, 2))
    for branch in ("col", "sweep", "dense"):
        assert has(auto=branch)
    assert any(v["sel"] == "first" for v in V) and any(v["sel"] == "last" for v in V)
    assert any(v["H"] % 4 and v["bwd"] == "map_tok" for v in V) and any(v["T"] % 8 and v["bwd"] == "map_col" for v in V)
    qk = [v for v in V if v["kind"] == "qk"]
    assert {v["d"] for v in qk} == {5, 8, 40, 64} and {v["Bk"] for v in qk} == {1, 2} and {v["T"] for v in qk} == {13, 77}
    assert {v["sides"] for v in qk} == {(5,), (8, 16)}
    # which families run where: all of them on the token axis and on one variant per route
    for v in V:
        if v["name"].startswith("tok-axis") and v["T"] in (1, 16, 17, 77, 100, 128):
            assert set(v["families"]) == set(A._families(v["T"], A.FAMILIES))
    for route in ("map_groups", "map_wide"):
        assert any(v["fwd"] == route and set(v["families"]) == set(A.FAMILIES) for v in V)
    for route in ("map_dense_groups", "map_col", "map_tok"):
        assert any(v["bwd"] == route and set(v["families"]) == set(A.FAMILIES) for v in V)


SIDE_SETS = [(4,), (8,), (16,), (32,), (64,), (24,), (4, 8), (8, 16), (16, 32), (32, 64), (16, 16, 16, 32), (4, 8, 16, 32), (1, 2), (12, 40)]


def test_restated_plans_agree_with_the_library_over_a_sweep_of_shapes(tune):
    """skp_attn_map_fwd_wide_ok, _bwd_col_ok, _bwd_workspace, _bwd_col_workspace and _bwd_sparse_workspace (whose size encodes the
    band count) against the restatement of _map_cases.py."""
    from stablekeypoints_amd import _native as N
    lib = N.lib()
    n = 0
    for sides, T, R in itertools.product(SIDE_SETS, (1, 13, 77, 128, 129, 192, 193, 500, 1024, 1025), (6, 32, 48, 64, 96, 100, 128, 256, 320, 512, 2048, 4128)):
        si, _keep = N.int_array(sides)
        L = len(sides)
        assert bool(lib.skp_attn_map_fwd_wide_ok(si, L, T, R)) == (A.wide_plan(sides, T, R)[0] == 0), (sides, T, R)
        for B, H in ((1, 1), (2, 5), (8, 8)):
            assert lib.skp_attn_map_bwd_workspace(si, L, B, H, min(T, 128), R) == A.dense_workspace(sides, B, H, min(T, 128), R)
            for K in (1, 10, 16, 17, 32, 33):
                assert lib.skp_attn_map_bwd_col_ok(si, L, H, T, R, K) == A.col_ok(sides, H, T, R, K), (sides, H, T, R, K)
                assert lib.skp_attn_map_bwd_col_workspace(si, L, B, H, T, R, K) == A.col_workspace(sides, B, H, T, R, K)
                for forced in (0, 1, 3):
                    tune("map_bands", forced)
                    assert lib.skp_attn_map_bwd_sparse_workspace(si, L, B, H, T, R, K) == A.sparse_workspace(sides, B, H, T, R, K, forced), \
                        (sides, B, H, T, R, K, forced)
                    n += 1
    assert n > 10000


def test_checker_accepts_the_references_and_rejects_planted_defects():
    """assert_map_close passes the fp64 reference (any factor) and the fp32 reference (factor 1), and fails -- at the largest
    factor in use -- on the defects the families exist for: a pad column in the softmax sum, a token group dropped from the
    log-sum-exp, a border tap clamped one pixel short, the halo of one band not summed."""
    m = max(A.M.values())
    v = A.BY_NAME["tok-axis-T77"]
    for family in ("all_low", "randn"):
        c = A.case(v, family)
        A.assert_map_close({k: x for k, x in c.ref64.items()}, c, "fp64 itself", m=m)
        A.assert_map_close({k: x for k, x in c.ref32.items()}, c, "fp32 reference", m=1)
    # a spiked token with a map gradient: its own logits gradient is pure cancellation, and neither no gradient at all, nor one
    # five times too large, nor 1e-3 of the cancelling terms left standing may pass
    for name in ("tok-axis-T77", "groups-T200", "wide-T300"):
        vs = A.BY_NAME[name]
        c = A.case(vs, "spike_last")
        assert c.spike == vs["T"] - 1
        A.assert_map_close({"dS": [d.clone() for d in c.ref64["dS"]]}, c, "fp64 itself", m=m)
        A.assert_map_close({"dS": [d.clone() for d in c.ref32["dS"]]}, c, "fp32 reference", m=1)
        left = [d.clone() for d in c.ref64["dS"]]
        left[0][..., c.spike] += 1e-3 * c.cancel_scale
        for wrong in ([torch.zeros_like(d) for d in c.ref64["dS"]], [5 * d for d in c.ref64["dS"]], left):
            with pytest.raises(AssertionError):
                A.assert_map_close({"dS": wrong}, c, "wrong gradient on a spike", m=m)
    # pad columns (logit 0) in the sum: all_low sees it, randn at T = 77 may not
    c = A.case(v, "all_low")
    S_pad = [S.clone() for S in c.S]
    z = [torch.cat([S[..., :77], S[..., 77:78]], -1) for S in S_pad]
    bad = A.reference(z, v["sides"], v["H"], 78, v["R"], torch.cat([c.dM, torch.zeros_like(c.dM[:, :1])], 1), None, None, torch.float64)
    with pytest.raises(AssertionError):
        A.assert_map_close({"M": bad["M"][:, :77], "lse": bad["lse"]}, c, "pad column in the sum", m=m)
    # the last token group left out of the log-sum-exp: ramp puts the mass there
    v2 = A.BY_NAME["groups-T200"]
    c = A.case(v2, "ramp")
    part = A.reference([S[..., :192] for S in c.S], v2["sides"], v2["H"], 192, v2["R"], c.dM[:, :192], None, None, torch.float64)
    with pytest.raises(AssertionError):
        A.assert_map_close({"lse": part["lse"]}, c, "group dropped", m=m)
    # a border tap one pixel short (the last up-res row takes the taps of the row before it) in one layer, on the border family
    v3 = A.BY_NAME["sweep-mixed-R32-T77-K4"]
    c = A.case(v3, "border")
    R, H = v3["R"], v3["H"]

    def map_by_taps(short_layer):
        acc = 0
        for l, (z, s) in enumerate(zip(c.logits64(), v3["sides"])):
            W = A.tap_matrix(s, R)
            Wy = W.clone()
            if l == short_layer:
                Wy[-1] = W[-2]
            up = torch.einsum("yi,bhijt,xj->bhtyx", Wy, z.reshape(*z.shape[:2], s, s, -1), W)
            acc = acc + up.softmax(dim=2).sum(dim=1)
        return {"M": acc / (len(v3["sides"]) * H)}
    A.assert_map_close(map_by_taps(None), c, "the restated taps", m=1)
    with pytest.raises(AssertionError):
        A.assert_map_close(map_by_taps(1), c, "border tap one pixel short", m=m)
    # the seam gradient: dropping what one band adds to a halo row changes dS there by far more than the band allows
    c = A.case(v3, "randn")
    got = [d.clone() for d in c.ref64["dS"]]
    s = v3["sides"][3]
    r = (A.band_rows(R, v3["bands"])[0] * s) // R                         # the low-res row under the seam
    got[3].reshape(*got[3].shape[:2], s, s, -1)[:, :, r] *= 0.5
    with pytest.raises(AssertionError):
        A.assert_map_close({"dS": got}, c, "halo not summed", m=m)
